"""CPU checks of the batches test_pairhmm_f64_gpu.py runs (pairhmm_f64_cases.py): every test case lies where the GPU test needs it --
the ones meant for the fp64 re-run list inside the window (-560, THRESHOLD - 1) and flagged fp64 by the oracle, the ones meant to stay
fp32 above THRESHOLD + 1, the forced ones above -560 -- so that the GPU test needs no mask and no allowance; and the length lists reach
the fp64 kernels they claim, with and without MGX_PAIRHMM_MERGE_BELOW, as tests/cpp/pairhmm_plan_driver.cpp plans them with
csrc/pairhmm_plan.h.  The restatement of that header in pairhmm_f64_cases.py (f64_shapes) is compared with the driver on the same lists."""
import numpy as np
import pytest

import pairhmm_f64_cases as cases
from conftest import ROOT
from pairhmm_plan_cases import N_CU
from test_pairhmm_plan_host import PlanDriver

LOW, HIGH, KEEP = cases.LOW, cases.THRESHOLD - cases.MARGIN, cases.THRESHOLD + cases.MARGIN


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return PlanDriver(tmp_path_factory.mktemp("pairhmm_f64_plan"))


@pytest.fixture(scope="module")
def rec(oracle):          # `oracle` builds the library
    return cases.Recurrence(ROOT)


def test_window_constants():
    assert abs(cases.THRESHOLD - (-64.12)) < 0.005 and abs(cases.EXACT_BELOW - (-587.05)) < 0.005
    assert cases.EXACT_BELOW + 25 < LOW < HIGH < cases.THRESHOLD < KEEP


def in_window(oracle, d, meant=None):
    """every test case meant for the re-run list in the window and flagged fp64, every other one well above the threshold and flagged fp32"""
    want, wused = oracle.batch(d)
    meant = np.ones(len(want), dtype=bool) if meant is None else meant
    assert np.isfinite(want).all()
    assert (want[meant] > LOW).all() and (want[meant] < HIGH).all(), (want[meant].min(), want[meant].max())
    assert (want[~meant] > KEEP).all()
    assert np.array_equal(wused == 1, meant)
    return want


# ---- values -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,RPL", cases.CLASSES)
def test_forced_class_batches_stay_above_the_exact_tier(oracle, rec, G, RPL):
    d = cases.forced_class_batch(G, RPL)
    full, few = cases.class_lengths(G, RPL)
    assert d["n_pairs"] == cases.PER_CLASS and sorted(set(d["R"])) == sorted({full, few})
    assert (d["R"] == full).sum() == (d["R"] == few).sum() or full == few
    want, _ = cases.fp64_values(oracle, rec, d)
    assert np.isfinite(want).all() and want.min() > LOW
    # haplotypes shorter than the lane group, of its width, one more, and longer than the read: fill, drain and the guarded tail
    H = set(int(h) for h in d["H"])
    short = {h for h in (1, 2, G - 1, G, G + 1) if h >= 1}
    if full <= 330:
        assert short <= H
    assert len({h for h in H if h >= full}) >= 12


def test_default_threshold_batch_is_forced_material(oracle, rec):
    d, idx = cases.default_threshold_batch()
    assert d["n_pairs"] == 4100 and len(idx) == 64 and len(set(d["H"][idx])) > 8
    want, _ = cases.fp64_values(oracle, rec, cases.subset(d, idx))
    assert want.min() > LOW


@pytest.mark.parametrize("R", cases.STRIP_R)
def test_strip_batches(oracle, R):
    d = cases.strip_batch(R)
    assert d["n_pairs"] == 12 and (d["R"] == R).all()
    in_window(oracle, d)
    # a haplotype of one base and one of fewer than 64 survive next to reads of 1025 and 1040 bases only (cases.strip_short_haps)
    assert ({1, 40} <= set(int(h) for h in d["H"])) == (R <= 1100)
    for h in (1, 40):          # ... because beyond that they leave the window, even at a gap-continuation quality of 3
        if R > 1100:
            w, _ = oracle.batch(cases.short_hap_part(R, [h], 5))
            assert w[0] < LOW


@pytest.mark.parametrize("R", cases.RERUN_SHARED + cases.RERUN_OWN16 + cases.RERUN_OWN64)
def test_rerun_batches(oracle, R):
    d, meant = cases.rerun_batch(R, cases.RERUN_N, 0xCC00 + R)
    assert (d["R"] == R).all() and (~meant).sum() == cases.RERUN_N // 4 and len(set(d["H"])) > 8
    in_window(oracle, d, meant)


def test_wrap_batches(oracle):
    for d, n in ((cases.wrap_shared(N_CU), 32 * N_CU + 37), (cases.wrap_own64(N_CU), 8 * N_CU + 5), (cases.wrap_strip(N_CU), 4 * N_CU + 3)):
        assert d["n_pairs"] == n
        in_window(oracle, d)
        # later passes of the grid see other haplotype lengths than the first
        assert len(set(d["H"][:64])) > 4 and len(set(d["H"][-64:])) > 4


def test_shape_independence_batch(oracle):
    d = cases.shape_independence_batch()
    assert d["n_pairs"] == 64 and d["R"].min() == 8 and d["R"].max() == 128
    assert (d["gcp"] & 127).min() >= 1 and not (d["bases"] == ord("N")).any() and not (d["hap_bases"] == ord("N")).any()
    in_window(oracle, d)


@pytest.mark.parametrize("R", cases.CONTENT_R)
def test_content_batches(oracle, R):
    d = cases.content_batch(R)
    in_window(oracle, d)
    plain = cases.rerun_part(R, d["n_pairs"], 0xC0DE00 + R)
    names = [cases.CONTENT_NAMES[i % len(cases.CONTENT_NAMES)] for i in range(d["n_pairs"])]
    changed = [any(not np.array_equal(d[k][o[i]:o[i + 1]], plain[k][o[i]:o[i + 1]]) for k in cases.KEYS
                   for o in [(d["hap_off"] if k == "hap_bases" else d["read_off"]).astype(np.int64)]) for i in range(d["n_pairs"])]
    assert changed == [nm != "plain" for nm in names]
    assert (d["gcp"] == 0).any() and (d["gcp"] == 128).any() and ((d["ins"] == 0) & (d["dele"] == 0)).any()
    for k in ("qual", "ins", "dele", "gcp"):
        assert (d[k] >= 128).any()
    for k in ("bases", "hap_bases"):
        assert (d[k] == ord("N")).any() and (d[k] == ord("a")).any() and (d[k] == 0xFF).any() or R == 32   # 12 draws of 8 bytes


# ---- reach ----------------------------------------------------------------------------------------------------------------------------

def planned(driver, lengths, merge_below=None, min_g=4, haps=None):
    """the driver's plan of a batch of these read lengths -> (the classes' own fp64 shapes, the fp64 launches of a default run, plan)"""
    haps = list(haps) if haps is not None else [int(r) + 1 for r in lengths]
    p = driver.plan(list(map(int, lengths)), haps, pairs=[(i, i) for i in range(len(lengths))], n_cu=N_CU, min_g=min_g, merge_below=merge_below)
    assert p["rc"] == 0
    own = sorted({(64, 17) if b["strip"] else (b["Gd"], b["RPLd"]) for b in p["bins"]})
    runs = sorted({(64, 17) if ln[0] == "strip64" else (ln[1], ln[2]) for ln in p["launches"] if ln[0] in ("f64", "strip64")})
    return own, runs, p


def check_restatement(driver, lengths, merge_below, min_g=4):
    own, runs, p = planned(driver, lengths, merge_below, min_g)
    kw = dict(merge_below=merge_below or cases.K_MERGE_BELOW, min_g=min_g)
    assert cases.f64_shapes(lengths, True, **kw) == own
    assert cases.f64_shapes(lengths, False, **kw) == runs
    return own, runs, p


@pytest.mark.parametrize("G,RPL", cases.CLASSES)
def test_forced_class_batches_reach_their_class(driver, G, RPL):
    d = cases.forced_class_batch(G, RPL)
    own, _, p = check_restatement(driver, d["R"], 1, cases.NEED_MIN_G.get((G, RPL), 4))
    want = (64, 3) if (G == 16 and RPL > 8) else (G, RPL)          # the four classes of 16 lanes x 9..12 rows: one test case per wavefront
    assert own == [want] and len(p["bins"]) == 1 and (p["bins"][0]["G"], p["bins"][0]["RPL"]) == (G, RPL)
    # without the knob the class is folded into the widest of its lane width (or is that one)
    own_folded, _, _ = check_restatement(driver, d["R"], None, cases.NEED_MIN_G.get((G, RPL), 4))
    assert own_folded == [{4: (4, 8), 8: (8, 8), 16: (64, 3), 64: (64, 16)}[G]]


def test_every_fp64_kernel_is_claimed():
    """38 instantiations of pick_kernel<double> and the strip kernel: 36 are the own shape of a class (forced), <double, 64, 3> is that of four
    classes, and <double, 16, 1..4> are also what the shared launch takes for short reads"""
    f64 = {(g, r) for g in (4, 8, 16) for r in range(1, 9)} | {(64, r) for r in range(3, 17)}
    own = {bs[2:4] for bs in (cases.bin_shape(cases.bin_index(G, RPL)) for G, RPL in cases.CLASSES)}
    assert own == f64 and len(f64) == 38
    assert set(cases.CONTENT_KERNEL.values()) <= {cases.kernel_name(*s) for s in f64 | {(64, 17)}}


def test_4100_reads_of_320_reach_64x5_at_the_real_threshold(driver):
    own, runs, _ = check_restatement(driver, [320] * 4100, None)
    assert own == runs == [(64, 5)]
    assert planned(driver, [320] * 4095)[0] == [(64, 16)]


@pytest.mark.parametrize("R", cases.STRIP_R)
def test_strip_lengths_reach_the_strip_kernel(driver, R):
    for knob in (1, None):
        own, runs, _ = check_restatement(driver, [R] * 12, knob)
        assert own == runs == [(64, 17)]
    assert (R - 1) // 1024 + 1 == {1025: 2, 1040: 2, 2048: 2, 2049: 3, 2100: 3}[R]          # strips of 1024 rows


@pytest.mark.parametrize("R", cases.RERUN_SHARED + cases.RERUN_OWN16 + cases.RERUN_OWN64)
def test_rerun_lengths_reach_their_shape(driver, R):
    own, runs, p = check_restatement(driver, [R] * cases.RERUN_N, 1)
    assert runs == [cases.RERUN_EXPECT[R]]
    narrow = R <= 128
    assert (p["narrow"][1] == cases.RERUN_N) == narrow          # the shared list covers the batch, or there is none
    # without the knob the batch is folded into another class and takes another fp64 shape -- except where it is the widest class already
    _, folded, _ = check_restatement(driver, [R] * cases.RERUN_N, None)
    want = (16, 2) if R <= 32 else (16, 4) if R <= 64 else (64, 3) if R <= 192 else (64, 16)
    assert folded == [want]
    assert (folded != runs) == (R not in (17, 32, 64, 129, 192, 1024))


def test_lists_are_longer_than_one_pass_of_their_grid(driver, oracle):
    n = 32 * N_CU + 37
    d = cases.wrap_shared(N_CU)
    _, runs, p = check_restatement(driver, d["R"], None)
    shared = [ln for ln in p["launches"] if ln[0] == "f64"]          # 8 lanes x 5 rows, a class of its own at this size: 40 rows, 16 x 3
    assert runs == [(16, 3)] and len(shared) == 1 and shared[0][4] == 8 * N_CU and 4 * shared[0][4] < n          # four test cases per workgroup
    n = 8 * N_CU + 5
    _, runs, p = check_restatement(driver, [193] * n, None)
    assert runs == [(64, 16)] and p["bins"][0]["grid_f64"] == 8 * N_CU < n
    n = 4 * N_CU + 3
    d = cases.wrap_strip(N_CU)
    _, runs, p = check_restatement(driver, d["R"], None)
    assert runs == [(64, 17)] and p["bins"][0]["grid_f32"] == p["bins"][0]["grid_f64"] == 4 * N_CU < n
    d = cases.wrap_exact(N_CU)
    _, _, p = planned(driver, np.diff(d["read_off"].astype(np.int64)), None, haps=np.diff(d["hap_off"].astype(np.int64)))
    want, _ = oracle.batch(d)
    assert p["exact"][2] == 2 * N_CU < int((np.isinf(want) | (want < cases.EXACT_BELOW - 0.01)).sum())          # what the fp64 launch leaves to it


def test_shape_independence_ways(driver):
    """the ways of GPU test e take different fp64 shapes for the same read"""
    R = [int(r) for r in cases.shape_independence_batch()["R"]]
    one_by_one = sorted({s for r in R for s in cases.f64_shapes([r], False, 1)})
    ways = {"forced, own classes": cases.f64_shapes(R, True, 1), "forced, folded": cases.f64_shapes(R, True),
            "one by one, own classes": one_by_one, "next to 128, own classes": cases.f64_shapes(R + [128] * 16, False, 1),
            "next to 150, folded": cases.f64_shapes(R + [150] * 16, False), "together, folded": cases.f64_shapes(R, False),
            "queue of 7": sorted({s for i in range(0, 64, 7) for s in cases.f64_shapes(R[i:i + 7], False)})}
    for lens, knob in ((R, 1), (R, None), (R + [128] * 16, 1), (R + [150] * 16, None)) + tuple(([r], 1) for r in sorted(set(R))):
        check_restatement(driver, lens, knob)
    assert len(ways["forced, own classes"]) == 14 and ways["forced, folded"] == [(4, 8), (8, 8), (64, 3)]
    assert one_by_one == [(16, r) for r in range(1, 9)]          # the shared launch sized by the read's own rows
    assert ways["next to 128, own classes"] == [(16, 8)]
    assert ways["next to 150, folded"] == ways["together, folded"] == [(16, 4), (64, 3)]
    assert len({tuple(v) for v in ways.values()}) >= 5, ways
