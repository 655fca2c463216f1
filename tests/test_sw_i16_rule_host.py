"""The admission rule of the packed 16-bit Smith-Waterman fill (csrc/sw_i16_rule.h) on the CPU: tests/cpp/sw_i16_rule_driver.cpp under
AddressSanitizer + UBSan runs the rule next to a 64-bit restatement of what k_sw_fill16 computes for a pair's own matrix.
Soundness: nothing an admitted pair makes the kernel form leaves 16 bits, and the pair's stand-in for LOW_INIT_VALUE loses
wherever it meets a real value.  Bite: the inputs do come as near the rule's bounds as real sequences can.  Shape: admission is
monotone in both lengths, which is what lets the GPU test bisect for the frontier.  All integer-exact."""
import pytest

import sw_frontier as F


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return F.Driver(tmp_path_factory.mktemp("sw_i16_rule"), sanitize=True)


def assert_sound(res, bounds, what):
    """res: one model result; bounds: the rule's own figures for the pair's lengths"""
    assert res is not None, what
    assert -32768 <= res["amin"] and res["amax"] <= 32767, (what, res)                 # every value, low16 and low16 + extend included
    assert -32768 <= res["dmin"] and res["dmax"] <= 32767, (what, res)                 # every difference whose sign bit is taken
    assert res["margin"] > 0, (what, res)                                               # low16 + extend loses strictly to H + open
    assert res["wrong"] == 0, (what, res)                                               # H and the four decisions as with LOW_INIT_VALUE
    # and the rule's own claim, from which the three above follow
    assert bounds["lh"] - bounds["pad"] <= res["rmin"] and res["rmax"] <= bounds["up"] and bounds["ll"] <= res["amin"], (what, res, bounds)


def probe_box(driver, params, side, n_random):
    """every (n, m) of [1, side]^2: admission and monotonicity; the model on every admitted point within six steps of a refused one
    or with a length of 1 (extremal sequences under all strategies; `n_random` random pairs per strategy within two steps).
    -> (per-point bounds, frontier points, model results per point)"""
    pts = [(n, m) for n in range(1, side + 1) for m in range(1, side + 1)]
    B = dict(zip(pts, driver.admits(params, pts)))
    ok = lambda n, m: n <= side and m <= side and B[(n, m)]["ok"] == 1          # noqa: E731
    near = lambda n, m, k: all(ok(min(n + d, side), min(m + e, side)) for d in range(k + 1) for e in range(k + 1))          # noqa: E731
    for n, m in pts:                                                            # refused stays refused as either length grows
        if not ok(n, m):
            assert not ok(n + 1, m) and not ok(n, m + 1), (params, n, m)
    frontier = [p for p in pts if ok(*p) and max(p) < side and not (ok(p[0] + 1, p[1]) and ok(p[0], p[1] + 1))]
    lines, owner = [], []
    for n, m in pts:
        if not ok(n, m) or (min(n, m) > 1 and near(n, m, 6)):
            continue
        for st in F.STRATEGIES:
            for kind in F.EXTREMAL_KINDS:
                lines.append(F.model_pair_line(params, st, *F.extremal(kind, n, m))); owner.append((n, m))
            if n_random and not near(n, m, 2):
                lines.append(F.model_rand_line(params, st, n, m, n_random, 1000 * n + m)); owner.append((n, m))
    results = {}
    for p, line, res in zip(owner, lines, driver.model(lines)):
        assert_sound(res, B[p], (params, p, line[:60]))
        results.setdefault(p, []).append(res)
    return B, frontier, results


# Where a bound is loose by construction, so that no input reaches it to within one pad (the test prints the gap it observed):
LOOSE_LO = ("lh = b(max(n, m)) + min(n, m) * mismatch is the all-diagonal path from the boundary's farthest value.  H is the BEST "
            "path: where one gap costs less than the mismatches it replaces, the diagonal is never the best one, and a path that "
            "leaves the boundary at b(x) has max(n, m) - x rows left, not min(n, m) diagonal steps more")
LOOSE_HI = ("positive gaps: u0 = bhi + (n + m) * pos charges the boundary's highest value, which has already walked max(n, m) "
            "steps, and n + m further steps at the best rate of any step")
LOOSE = {
    "standard_ngs_x20": {"lo": LOOSE_LO}, "flat_x8": {"lo": LOOSE_LO}, "zero_extend": {"lo": LOOSE_LO},
    "match_below_mismatch": {"lo": LOOSE_LO}, "all_negative": {"lo": LOOSE_LO},
    "positive_open_and_extend": {"lo": LOOSE_LO, "hi": LOOSE_HI}, "positive_extend_only": {"lo": LOOSE_LO, "hi": LOOSE_HI},
}
# A loose bound refuses pairs that would have been safe; it admits none that is not.


@pytest.mark.parametrize("name,params,side", F.SCALED_SETS, ids=[s[0] for s in F.SCALED_SETS])
def test_soundness_and_bite_on_dense_boxes(driver, name, params, side):
    B, frontier, results = probe_box(driver, params, side, n_random=64)
    n_adm = sum(1 for b in B.values() if b["ok"])
    assert frontier and 0 < n_adm < len(B), "the frontier has to cut through the box"
    pad = B[(1, 1)]["pad"]
    gap_hi = min(B[p]["u0"] - max(r["rmax"] for r in results[p]) for p in frontier)
    gap_lo = min(min(r["rmin"] for r in results[p]) - B[p]["lh"] for p in frontier)
    print(f"{name} {params}: box {side}, {n_adm} admitted, {len(frontier)} frontier points, pad {pad}, "
          f"u0 - observed max = {gap_hi}, observed min - lh = {gap_lo}")
    loose = LOOSE.get(name, {})
    if "hi" in loose:
        assert gap_hi > pad, "no longer loose: drop the entry.  It said: " + loose["hi"]
    else:
        assert gap_hi <= pad, (gap_hi, pad)
    if "lo" in loose:
        assert gap_lo > pad, "no longer loose: drop the entry.  It said: " + loose["lo"]
    else:
        assert gap_lo <= pad, (gap_lo, pad)


@pytest.mark.parametrize("name,params,side", F.DEGENERATE_SETS, ids=[s[0] for s in F.DEGENERATE_SETS])
def test_soundness_where_the_stand_in_for_low_init_meets_its_neighbour(driver, name, params, side):
    """match = mismatch = extend = 0: lo = 2 * open is reached by H(i, 0) + open, so low16 loses by the rule's "- 1" alone.
    Every short pair is admitted (nothing grows with the lengths): no frontier here, only the strictness."""
    B, frontier, results = probe_box(driver, params, side, n_random=0)
    assert all(b["ok"] for b in B.values())
    assert min(r["margin"] for rs in results.values() for r in rs) == 1


@pytest.mark.parametrize("params", F.REAL_SETS, ids=str)
def test_soundness_at_the_frontier_of_the_real_parameters(driver, params):
    """the parameter sets callers use, at the lengths the GPU test runs: for a reference at the top of a few row classes, the
    largest admitted alternate, found by bisection; extremal sequences under every strategy"""
    lines, bounds = [], []
    for n in (1, 64, 200, 1000, 2048):
        m = driver.largest_admitted_alt(params, n)
        if m == 0:
            continue
        a, r = driver.admits(params, [(n, m), (n, m + 1)])
        assert a["ok"] == 1 and r["ok"] == 0
        for k, kind in enumerate(F.EXTREMAL_KINDS):
            if n > 200 and k % 2:
                continue
            for st in (F.STRATEGIES if n <= 200 else (F.STRATEGIES[(k // 2) % 4],)):
                lines.append(F.model_pair_line(params, st, *F.extremal(kind, n, m))); bounds.append(a)
    assert lines
    for line, b, res in zip(lines, bounds, driver.model(lines)):
        assert_sound(res, b, (params, line[:60]))


def test_lds_limit_of_the_alternate(driver):
    """4096 bases admitted, 4097 refused, for parameters whose score bound allows both.  (3, -1, -4, -3) with a 200-base
    reference, by hand: blo = -4 - 4095 * 3 = -12289, lh = blo - 200 = -12489, pad = 10, low = lh - 10 - 3 - 1 = -12503,
    ll = -12506; up = 200 * 3 + 10 = 610."""
    for n in (1, 200, 2048):
        a, b, c = driver.admits(F.ORIGINAL_DEFAULT, [(n, 4095), (n, 4096), (n, 4097)])
        assert (a["ok"], b["ok"], c["ok"]) == (1, 1, 0)
        assert c["ll"] >= -32768 and c["up"] - c["ll"] <= 32767              # refused by the length alone
    b = driver.admits(F.ORIGINAL_DEFAULT, [(200, 4096)])[0]
    assert (b["ll"], b["up"], b["low16"]) == (-12506, 610, -12503)
    assert driver.largest_admitted_alt(F.ORIGINAL_DEFAULT, 200) == 4096
