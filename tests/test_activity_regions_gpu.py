"""mgx_activity_profile_regions (include/mgx_activity.h) on the device, through the C ABI: for every case of activity_region_cases.py the
regions equal and every state value bit-equal to what the reference's compiled ActivityProfile.cpp gave (tests/golden/
activity_regions.npz, its weights passed in) and to the statement-by-statement restatement of its streaming code; the library's own
default weights; every argument error with nothing launched; the overflow codes and the counts they report; the stats; and the fused
mgx_activity_interval_regions against the two calls it fuses.  No case and no state is left out of a comparison."""
import ctypes
import errno
import os

import numpy as np
import pytest

import activity_cases as A
import activity_region_cases as R

pytestmark = pytest.mark.gpu
CASES = R.all_cases()


@pytest.fixture(scope="module")
def act(pkg):
    e = pkg.ActivityEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activity_regions.npz"))
    assert int(g["digest"][0]) == R.digest(CASES), "the fixture was made from other cases: run tests/golden/make_golden_activity_regions.py"
    return g


@pytest.fixture(scope="module")
def default_weights(golden):
    """the reference's own, passed in: this machine's libm stays out of the comparisons"""
    return golden["weights"]


def sizes(c):
    p = c["params"]
    return dict(max_prob_propagation=p["max_prob_propagation"], active_prob_threshold=p["active_prob_threshold"], padding=p["padding"],
                min_region_size=p["min_region_size"], max_region_size=p["max_region_size"])


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_every_case_equals_the_reference_and_the_restatement(act, golden, default_weights, k):
    c = CASES[k]
    w = R.weights_of(c, default_weights)
    regions, values = act.profile_regions(c["interval_start"], c["prob"], c["contig_length"], weights=w, **sizes(c))
    r0, r1, s0, s1 = (int(golden[n][k + d]) for n in ("region_off", "state_off") for d in (0, 1))
    assert np.array_equal(regions, golden["regions"][r0:r1]), (c["name"], regions[:6].tolist(), golden["regions"][r0:r1][:6].tolist())
    assert len(values) == s1 - s0 and np.array_equal(values.view(np.uint64), golden["values"][s0:s1].view(np.uint64)), c["name"]
    want_regions, want_values = R.restated(c, w)
    assert len(values) == len(want_values), (c["name"], len(values), len(want_values))
    differ = np.flatnonzero(values.view(np.uint64) != want_values.view(np.uint64))
    assert len(differ) == 0, (c["name"], differ[:8], values[differ[:4]], want_values[differ[:4]])
    assert np.array_equal(regions, want_regions), (c["name"], regions[:6].tolist(), want_regions[:6].tolist())
    st = act.region_stats()
    assert (st["n_states"], st["n_regions"]) == (len(want_values), len(want_regions)), st
    runs = int(np.sum(np.diff(np.concatenate([[0], (want_values > c["params"]["active_prob_threshold"]).astype(np.int8)])) == 1))
    assert st["n_runs"] == runs and st["n_launches"] == (10 if len(want_regions) else 9), (st, runs)


def test_the_librarys_own_weights(act, default_weights):
    """band_weights NULL: the library's weights (this host's libm) are within 4 ulp of the reference's, and the regions are those of the
    restatement run with the library's own weights"""
    own, f = act.band_weights()
    assert f == 50 and len(own) == 101
    ulp = np.abs(own.view(np.int64) - default_weights.view(np.int64)).max()
    assert ulp <= 4, ulp
    c = R.body_case()
    regions, values = act.profile_regions(c["interval_start"], c["prob"], c["contig_length"], **sizes(c))
    want_regions, want_values = R.restated(c, own)
    assert np.array_equal(regions, want_regions) and np.array_equal(values.view(np.uint64), want_values.view(np.uint64))
    assert len(regions) >= 5


def test_the_profile_is_optional_and_timing_fills_the_stats(act, default_weights, pkg):
    c = R.body_case()
    regions, values = act.profile_regions(c["interval_start"], c["prob"], c["contig_length"], weights=default_weights, profile=False, flags=pkg.activity.TIMING, **sizes(c))
    assert values is None and np.array_equal(regions, R.restated(c, default_weights)[0])
    st = act.region_stats()
    assert st["ms_band"] > 0 and st["ms_cut"] > 0


def test_argument_errors_launch_nothing(act, pkg):
    good = dict(interval_start=1000, prob=np.array([0.0, 1.0, 0.5, 0.0]), contig_length=2000)
    E = -errno.EINVAL

    def rc_of(weights=None, **kw):
        args = dict(good)
        over = {k: kw.pop(k) for k in list(kw) if k in args}
        args.update(over)
        rc = act.profile_regions_rc(args["interval_start"], args["prob"], args["contig_length"], weights=weights, **kw)[0]
        return rc, act.region_stats()
    assert rc_of()[0] == 0 and rc_of()[1]["n_launches"] >= 9
    cases = [
        ("max_prob_propagation below the filter size", dict(max_prob_propagation=49)),
        ("max_prob_propagation below a caller's filter size", dict(weights=[0.1] * 7, max_prob_propagation=2)),
        ("a NaN probability", dict(prob=np.array([0.0, np.nan]))),
        ("a probability above 1", dict(prob=np.array([0.0, 1.0000000000000002]))),
        ("a probability below 0", dict(prob=np.array([-1e-300, 1.0]))),
        ("min_region_size 0", dict(min_region_size=0)),
        ("max_region_size below min_region_size", dict(max_region_size=49)),
        ("contig_length at the last locus", dict(contig_length=1003)),
        ("an infinite threshold", dict(active_prob_threshold=float("inf"))),
        ("a NaN threshold", dict(active_prob_threshold=float("nan"))),
        ("sigma 0", dict(sigma=0.0)),
        ("sigma negative", dict(sigma=-1.0)),
        ("a filter size above the cap", dict(max_filter_size=pkg.activity.MAX_FILTER + 1, adaptive_filter_size=0, max_prob_propagation=1000)),
        ("caller's weights above the cap", dict(weights=[0.001] * (2 * pkg.activity.MAX_FILTER + 3), max_prob_propagation=1000)),
        ("an even number of weights", dict(weights=[0.5, 0.5])),
        ("a weight that is not finite", dict(weights=[0.25, float("inf"), 0.25])),
        ("negative padding", dict(padding=-1)),
    ]
    for name, kw in cases:
        rc, st = rc_of(**kw)
        assert rc == E, (name, rc, pkg.native.load().mgx_last_error())
        assert st["n_launches"] == 0 and st["n_states"] == 0, (name, st)
    # NULL pointers
    lib = pkg.native.load()
    rp, _ = act.region_params()
    n = ctypes.c_uint64(0)
    out = np.zeros((4, 4), np.int32)
    prob = good["prob"]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.mgx_activity_profile_regions(act.ctx, 1000, 4, None, 2000, ctypes.byref(rp), P(out), 4, ctypes.byref(n), None, 0, ctypes.byref(n)) == E
    assert lib.mgx_activity_profile_regions(act.ctx, 1000, 4, P(prob), 2000, None, P(out), 4, ctypes.byref(n), None, 0, ctypes.byref(n)) == E
    assert lib.mgx_activity_profile_regions(act.ctx, 1000, 4, P(prob), 2000, ctypes.byref(rp), None, 4, ctypes.byref(n), None, 0, ctypes.byref(n)) == E
    assert lib.mgx_activity_profile_regions(act.ctx, 1000, 4, P(prob), 2000, ctypes.byref(rp), P(out), 4, None, None, 0, ctypes.byref(n)) == E
    assert act.region_stats()["n_launches"] == 0
    # the context still works, and a contig that ends right behind the last locus is fine
    rc, regions, values, (n_regions, n_states) = act.profile_regions_rc(1000, prob, 1004)
    assert rc == 0 and n_states == 4 and n_regions == 1 and regions[0].tolist() == [1000, 1003, 900, 1003]


def test_overflow_reports_the_counts_and_writes_nothing(act, default_weights):
    c = R.body_case()
    want_regions, want_values = R.restated(c, default_weights)
    n = len(want_regions)
    rc, regions, values, counts = act.profile_regions_rc(c["interval_start"], c["prob"], c["contig_length"], weights=default_weights, cap=n - 1, **sizes(c))
    assert rc == -errno.ENOSPC and counts == (n, len(want_values)) and (regions == -1).all() and (values == -1.0).all()
    rc, regions, values, counts = act.profile_regions_rc(c["interval_start"], c["prob"], c["contig_length"], weights=default_weights, profile_cap=len(want_values) - 1, **sizes(c))
    assert rc == -errno.ENOSPC and counts == (n, len(want_values)) and (regions == -1).all() and (values == -1.0).all()
    rc, regions, values, counts = act.profile_regions_rc(c["interval_start"], c["prob"], c["contig_length"], weights=default_weights, cap=n, profile_cap=len(want_values), **sizes(c))
    assert rc == 0 and np.array_equal(regions[:n], want_regions)


def test_no_loci(act):
    rc, regions, values, counts = act.profile_regions_rc(5, np.zeros(0), 100)
    assert rc == 0 and counts == (0, 0) and act.region_stats()["n_launches"] == 0


def fused_inputs():
    shapes = {c["name"]: c for c in A.shape_cases()}
    return [A.body_case(), shapes["interval of 130 loci"], shapes["cigar 151M"]]


@pytest.mark.parametrize("k", range(3))
def test_the_fused_call_equals_the_two_calls_it_fuses(act, default_weights, k):
    c = fused_inputs()[k]
    d = c["input"]
    contig = int(d["interval_start"]) + len(d["ref_bases"]) + 1000
    active, log_odds, depth = act.interval(d, **c["params"])
    want_regions, want_values = act.profile_regions(d["interval_start"], active.astype(np.float64), contig, weights=default_weights)
    regions, values, loci = act.interval_regions(d, contig, weights=default_weights, **c["params"])
    assert np.array_equal(regions, want_regions) and np.array_equal(values.view(np.uint64), want_values.view(np.uint64)), c["name"]
    assert np.array_equal(loci[0], active) and np.array_equal(loci[1], log_odds, equal_nan=True) and np.array_equal(loci[2], depth), c["name"]
    st, rst = act.stats(), act.region_stats()
    assert st["n_active"] == int(active.sum()) and st["n_launches"] == 2 and rst["n_regions"] == len(want_regions) and rst["n_states"] == len(want_values)
    # without the per-locus outputs, and without the profile
    regions, values, loci = act.interval_regions(d, contig, weights=default_weights, per_locus=False, **c["params"])
    assert loci is None and np.array_equal(regions, want_regions) and np.array_equal(values.view(np.uint64), want_values.view(np.uint64)), c["name"]
    regions, values, loci = act.interval_regions(d, contig, weights=default_weights, per_locus=False, profile=False, **c["params"])
    assert values is None and np.array_equal(regions, want_regions), c["name"]
    if k == 0:
        assert len(want_regions) >= 3 and int(active.sum()) >= 10


def test_the_fused_calls_argument_errors_launch_nothing(act, default_weights):
    c = A.body_case()
    d = c["input"]
    contig = int(d["interval_start"]) + len(d["ref_bases"]) + 1000
    E = -errno.EINVAL
    bad_reads = dict(d)
    bad_reads["sample"] = d["sample"].copy()
    bad_reads["sample"][1] = 2
    for name, rc in (("region parameters", act.interval_regions_rc(d, contig, region_params=dict(max_prob_propagation=49), **c["params"])[0]),
                     ("contig_length", act.interval_regions_rc(d, int(d["interval_start"]) + len(d["ref_bases"]) - 1, **c["params"])[0]),
                     ("the reads", act.interval_regions_rc(bad_reads, contig, **c["params"])[0]),
                     ("the per-locus parameters", act.interval_regions_rc(d, contig, **dict(c["params"], pcr_error_qual=1))[0])):
        assert rc == E, (name, rc)
        assert act.stats()["n_launches"] == 0 and act.region_stats()["n_launches"] == 0, name
    want = act.interval_regions(d, contig, weights=default_weights, **c["params"])[0]
    rc, regions, values, loci, counts = act.interval_regions_rc(d, contig, weights=default_weights, cap=len(want) - 1, **c["params"])
    assert rc == -errno.ENOSPC and counts[0] == len(want) and (regions == -1).all()
