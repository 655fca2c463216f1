"""mgx_activity_interval (include/mgx_activity.h) on the device, through the C ABI: activity, depth and element bytes exactly and the
log-odds within 1e-9 against the sequential restatement of the reference (activity_cases.py) and against the reference's own answers
(tests/golden/activity.npz), at the kernels' seams and on a seeded body of reads; every argument error with nothing launched; the
depth limit; and the same reads over an interval and over its two halves.  No locus is left out of any comparison: the cases hold none
whose log-odds lies within 1e-6 of the threshold (tests/test_activity_host.py asserts that on the CPU)."""
import ctypes
import errno
import os

import numpy as np
import pytest

import activity_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = A.shape_cases()


@pytest.fixture(scope="module")
def act(pkg):
    e = pkg.ActivityEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "activity.npz"))
    assert int(g["digest"][0]) == A.digest(SHAPES + [A.body_case()]), "the fixture was made from other cases: run tests/golden/make_golden_activity.py"
    return g


def check(act, c, golden=None, k=None):
    active, log_odds, depth = act.interval(c["input"], **c["params"])
    w_el, w_active, w_lo, w_depth, w_callable = A.restated(c)
    wants = [(w_el, w_active, w_lo, w_depth)]
    if golden is not None:
        e0, e1, l0, l1 = (int(golden[n][k + d]) for n in ("elem_off", "locus_off") for d in (0, 1))
        wants.append((golden["elements"][e0:e1], golden["active"][l0:l1], golden["log_odds"][l0:l1], golden["depth"][l0:l1]))
    el = act.last_elements()
    for which, (g_el, g_active, g_lo, g_depth) in zip(("restatement", "reference"), wants):
        assert np.array_equal(el, g_el), (c["name"], which, np.flatnonzero(el != g_el)[:8] if len(el) == len(g_el) else (len(el), len(g_el)))
        assert np.array_equal(depth, g_depth), (c["name"], which)
        assert np.array_equal(np.isnan(log_odds), np.isnan(g_lo)), (c["name"], which)
        err = float(np.nanmax(np.abs(log_odds - g_lo), initial=0.0))
        print("%s vs %s: max |log-odds difference| %.3g over %d loci" % (c["name"], which, err, int((~np.isnan(g_lo)).sum())))
        assert err <= A.LOG_ODDS_TOL, (c["name"], which, err)
        assert np.array_equal(active, g_active), (c["name"], which, np.flatnonzero(active != g_active)[:8])
    st = act.stats()
    assert (st["n_loci"], st["n_elements"], st["n_active"], st["n_callable"]) == (len(w_active), len(w_el), int(w_active.sum()), w_callable), (c["name"], st)
    assert st["n_launches"] == (2 if len(w_el) else 1)
    return active, log_odds, depth


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[c["name"] for c in SHAPES])
def test_the_shapes(act, golden, k):
    check(act, SHAPES[k], golden, k)


def test_a_body_of_reads(act, golden):
    c = A.body_case()
    active, log_odds, _ = check(act, c, golden, len(SHAPES))
    assert len(c["input"]["read_start"]) == 2000 and len(active) == 3000 and int(active.sum()) >= 10 and int(np.isnan(log_odds).sum()) >= 100


def test_the_same_reads_over_an_interval_and_over_its_halves(act):
    c = A.cut_case()
    d = c["input"]
    whole = act.interval(d, **c["params"])
    w_active, w_lo = A.restated(c)[1:3]
    assert np.array_equal(whole[0], w_active) and float(np.nanmax(np.abs(whole[1] - w_lo))) <= A.LOG_ODDS_TOL
    n = len(d["ref_bases"])
    for b in (1, 64, 333, n - 1):
        left, right = act.interval(A.sub_interval(d, 0, b), **c["params"]), act.interval(A.sub_interval(d, b, n), **c["params"])
        for k in range(3):
            assert np.array_equal(np.concatenate([left[k], right[k]]), whole[k], equal_nan=True), (b, k)
    assert int((~np.isnan(whole[1])).sum()) >= 50


def broken(d, **changes):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    for k, v in changes.items():
        if callable(v):
            v(out[k])
        else:
            out[k] = v
    return out


def put(index, value):
    def f(a):
        a[index] = value
    return f


def test_argument_errors_launch_nothing(act, pkg):
    good = A.case("good", (1100, 40), [A.read(1100, "5M2D5M"), A.read(1104, "3S7M", mism=(4,)), A.read(1110, "10M")])["input"]
    E, B = -errno.EINVAL, -errno.E2BIG
    long_d = [(1 << 4) | A.M] + [(268435455 << 4) | A.D] * 6 + [(1 << 4) | A.M]
    huge = A.synth.pack_activity_reads(0, b"ACGT", [dict(start=0, cigar=long_d, bases=b"AC", quals=[30, 30]) for _ in range(3)])
    cases = [
        ("cigar_off decreases", broken(good, cigar_off=put(1, 7)), E),
        ("base_off decreases", broken(good, base_off=put(2, 3)), E),
        ("act_start not sorted", broken(good, act_start=put(2, 1103), act_stop=put(2, 1103)), E),
        ("window starts before the read", broken(good, act_start=put(0, 1099)), E),
        ("window ends behind the read", broken(good, act_stop=put(2, 1120)), E),
        ("operator code 9", broken(good, cigar=put(0, (5 << 4) | 9)), E),
        ("operator N", broken(good, cigar=put(1, (2 << 4) | A.N)), E),
        ("zero-length element", broken(good, cigar=put(1, A.D)), E),
        ("CIGAR read length is not the number of bases", broken(good, cigar=put(0, (6 << 4) | A.M), act_stop=put(0, 1100)), E),
        ("quality 128", broken(good, quals=put(7, 128)), E),
        ("sample 2", broken(good, sample=put(1, 2)), E),
        ("2^32 pileup elements", huge, B),
        ("interval beyond 2^31", broken(good, interval_start=2 ** 31 - 8, act_start=np.full(3, 5, np.int32), act_stop=np.full(3, 4, np.int32)), B),
    ]
    assert act.interval_rc(good)[0] == 0 and act.stats()["n_launches"] == 2
    for name, d, want in cases:
        rc, active, log_odds, depth = act.interval_rc(d)
        st = act.stats()
        assert rc == want, (name, rc, pkg.native.load().mgx_last_error())
        assert st["n_launches"] == 0 and st["n_loci"] == 0 and st["n_elements"] == 0, (name, st)
        assert (active == 255).all() and (log_odds == -1.0).all(), name
    for name, par in (("pcr_error_qual 1", dict(pcr_error_qual=1)), ("min_base_quality 128", dict(min_base_quality=128))):
        assert act.interval_rc(good, **par)[0] == E and act.stats()["n_launches"] == 0, name
    # NULL pointers, through the structure itself
    lib = pkg.native.load()
    out = np.zeros(40, np.uint8)
    for field in ("ref_bases", "read_start", "cigar_off", "cigar", "base_off", "bases", "quals", "flags", "mate_start", "sample", "act_start", "act_stop"):
        inp, hold = pkg.activity.make_input(good)
        setattr(inp, field, None)
        assert lib.mgx_activity_interval(act.ctx, ctypes.byref(inp), ctypes.byref(act.params()), out.ctypes.data_as(ctypes.c_void_p), None, None) == E, field
        assert act.stats()["n_launches"] == 0, field
    inp, hold = pkg.activity.make_input(good)
    assert lib.mgx_activity_interval(act.ctx, ctypes.byref(inp), ctypes.byref(act.params()), None, None, None) == E
    assert lib.mgx_activity_interval(act.ctx, None, ctypes.byref(act.params()), out.ctypes.data_as(ctypes.c_void_p), None, None) == E
    assert lib.mgx_activity_interval(act.ctx, ctypes.byref(inp), None, out.ctypes.data_as(ctypes.c_void_p), None, None) == E
    # the optional outputs may be NULL, and the context still works
    assert lib.mgx_activity_interval(act.ctx, ctypes.byref(inp), ctypes.byref(act.params()), out.ctypes.data_as(ctypes.c_void_p), None, None) == 0
    assert np.array_equal(out, act.interval(good)[0])


def test_a_locus_deeper_than_max_depth(pkg):
    e = pkg.ActivityEngine(0, max_depth=8)
    try:
        nine = A.case("nine", (1100, 12), [A.read(1100 + (k == 8), "10M", mism=(3,)) for k in range(9)])["input"]
        rc, active, log_odds, depth = e.interval_rc(nine)
        assert rc == -errno.E2BIG, (rc, pkg.native.load().mgx_last_error())
        assert (active == 255).all() and (log_odds == -1.0).all() and (depth == 0xFFFFFFFF).all()          # no partial result
        eight = A.case("eight", (1100, 12), [A.read(1100 + (k == 7), "10M", mism=(3,)) for k in range(8)])
        active, log_odds, depth = e.interval(eight["input"])
        w = A.restated(eight)
        assert np.array_equal(active, w[1]) and np.array_equal(depth, w[3]) and depth.max() == 8
        assert float(np.nanmax(np.abs(log_odds - w[2]))) <= A.LOG_ODDS_TOL
    finally:
        e.close()
