"""What can be said on the CPU about the batches of pairhmm_handoff_cases.py (the GPU tests of the five-operation sweep's lane hand-off):
that they reach the classes and the numbers of lanes in use they are named for, as csrc/pairhmm_plan.h folds them (restated in
pairhmm_f64_cases.py, which test_pairhmm_f64_host.py holds against the header), and that every test case but the ones deferred on
purpose stays with the five-operation cell AND in fp32, well above the float-first threshold, by the oracle and by the host emulation
of that cell (which takes the last-row sum from csrc/pairhmm_cell.h as the kernel does)."""
import numpy as np
import pytest

import pairhmm_handoff_cases as cases
from pairhmm_fiveop_cases import FIVE, HAP_N, STATIC, emulate
from test_pairhmm_oracle import assert_log10_close


@pytest.mark.parametrize("min_g", cases.MIN_GS)
def test_batches_reach_their_classes(min_g):
    seen = {}
    for name, knob, d in cases.batches(min_g):
        got = cases.classes_of(d, knob, min_g)
        for (G, RPL), _ in got.items():
            seen.setdefault((G, RPL), set()).update(cases.lanes(int(R), RPL) for R in d["R"]
                                                     if cases.f64.shape_of(int(R), min_g)[0] == G and cases.f64.shape_of(int(R), min_g)[1] <= RPL)
        if name.startswith("own_"):
            assert list(got) == [tuple(int(x) for x in name[4:].split("x"))] and d["n_pairs"] <= 64
        elif name.startswith(("folded_into_", "short_reads_in_")):
            assert list(got) == [tuple(int(x) for x in name.split("_")[-1].split("x"))], (name, got)
        elif name == "all_classes_one_batch":
            assert sorted(got) == sorted(cases.OWN[min_g])
        elif "4x8" in name or "8x8" in name:
            assert list(got) == [(4, 8)] or list(got) == [(8, 8)]
        else:
            assert list(got) == [(16, 8)] and d["n_pairs"] <= 4          # one wavefront
    want = {4: {(4, 1): {1, 2, 3, 4}, (4, 8): {1, 2, 3, 4}, (8, 8): {5, 6, 7, 8}, (16, 7): {15, 16}, (16, 8): {15, 16}, (16, 12): {6, 9, 14, 15, 16}},
            8: {(8, 1): {1, 2, 7, 8}, (8, 2): {7, 8}, (8, 8): {1, 2, 3}},
            16: {(16, 1): {1, 2, 15, 16}, (16, 2): {15, 16}, (16, 7): {1, 2, 16}, (16, 8): {1, 2, 16}, (16, 12): {1, 2}}}[min_g]
    for cls, nls in want.items():
        assert nls <= seen[cls], (cls, seen[cls])


def test_every_test_case_meant_for_the_sweep_stays_fp32(oracle):
    """Batch by batch: every test case but the ones deferred on purpose goes the five-operation way in the emulation, and its value lies
    at least 1 above the float-first threshold by the oracle and by the emulation, which agree on it.  So on the device its out_log10 is
    the five-operation sweep's own fp32 result, not an fp64 re-run's, and the recorded bytes hold the sweep to account."""
    for min_g in cases.MIN_GS:
        for name, _, d in cases.batches(min_g):
            mask = cases.five_mask(name, d) if name != "all_classes_one_batch" else np.ones(d["n_pairs"], dtype=bool)
            want, wused = oracle.batch(d)
            got, used, way = emulate(d)
            assert (way[mask] == FIVE).all(), (min_g, name, np.flatnonzero(mask & (way != FIVE)))
            assert np.isin(way[~mask], (HAP_N, STATIC)).all()
            assert not wused[mask].any() and not used[mask].any(), (min_g, name, np.flatnonzero(mask & ((wused | used) != 0)))
            low = min(want[mask].min(), got[mask].min())
            assert low > cases.f64.THRESHOLD + cases.f64.MARGIN, (min_g, name, low)
            assert_log10_close(got[mask], want[mask])
