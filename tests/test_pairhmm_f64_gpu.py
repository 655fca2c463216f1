"""GPU tests of the PairHMM fp64 tier: every kernel shape of pick_kernel<double> and the strip kernel in a launch of its
own, and every path that leads to them -- FORCE_DOUBLE (static job range, grid_f64_all), the re-run lists of the default engine (job_list,
a device-side count, a bounded grid that wraps over the list: the shared narrow list, a class's own list, the strip class's, the exact
tier's) and the queue.  Every value is compared with the fp64 recurrence itself (oracle/pairhmm_oracle.c, ph_oracle_prob_f64) at 1e-9,
the bar the project holds fp64 results to; -inf must equal -inf.  Each test prints the largest difference it saw.

The batches come from pairhmm_f64_cases.py; test_pairhmm_f64_host.py shows on the CPU that every test case lies at least 1 away from the
fp32 threshold and well above the exact tier, so that `used` equals the oracle's flags exactly and n_exact == 0, without mask or
allowance, and that the length lists reach the shapes named here.  MGX_PAIRHMM_MERGE_BELOW=1 ("the knob") keeps a class of 48 test cases
from being folded into the widest class of its lane width."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pairhmm_f64_cases as cases
from conftest import ROOT
from test_pairhmm_oracle import TOL

pytestmark = pytest.mark.gpu

BAR = cases.BAR
KNOB = "MGX_PAIRHMM_MERGE_BELOW"


def run(engine, d):
    b = engine.batch(d)
    b.run()
    out, used = b.results(with_flags=True)
    st = b.stats()
    b.close()
    return out, used, st


def report(what, diff):
    print(f"fp64 max diff [{what}]: {diff:.3e}")
    return diff


@pytest.fixture(scope="module")
def forced(pkg):
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.FORCE_DOUBLE | pkg.pairhmm.TIMING)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def rec(oracle):          # `oracle` builds the library
    return cases.Recurrence(ROOT)


@pytest.fixture(scope="module")
def n_cu():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a process of its own unless torch holds the device already: torch
    brings a HIP runtime of its own, which finds no device in a process where the library's runtime has opened it before"""
    import torch
    if torch.cuda.is_initialized():
        return torch.cuda.get_device_properties(0).multi_processor_count
    res = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, check=True, timeout=120)
    return int(res.stdout.split()[-1])


def check_forced(forced, oracle, rec, d, kernel, idx=None):
    out, used, st = run(forced, d)
    assert st["dominant_kernel"] == kernel and st["ms_f32_dominant"] == 0
    assert st["dominant_cells"] == d["cells"] and st["dominant_alg_bytes"] == d["alg_bytes"]
    assert used.all() and st["n_exact"] == 0 and st["n_rerun_f64"] == d["n_pairs"]
    sub = d if idx is None else cases.subset(d, idx)
    want, _ = cases.fp64_values(oracle, rec, sub)
    diff = report(kernel, cases.max_diff(out if idx is None else out[idx], want))
    assert diff < BAR
    return out


# ---- a. every fp64 shape in its own class, forced ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,RPL", [c for c in cases.CLASSES if c not in cases.NEED_MIN_G])
def test_every_shape_in_its_own_class_forced(forced, oracle, rec, monkeypatch, G, RPL):
    """48 test cases per fp32 class, half with every lane full and half with the most row-0 clones, haplotypes shorter than the lane group,
    of its width and longer than the read; the four classes of 16 lanes x 9..12 rows all run <double, 64, 3>."""
    monkeypatch.setenv(KNOB, "1")
    Gd, RPLd = cases.bin_shape(cases.bin_index(G, RPL))[2:4]
    assert (Gd, RPLd) == ((64, 3) if G == 16 and RPL > 8 else (G, RPL))
    check_forced(forced, oracle, rec, cases.forced_class_batch(G, RPL), cases.kernel_name(Gd, RPLd))


@pytest.mark.parametrize("min_g", [8, 16])
def test_narrow_shapes_that_need_min_g_forced(oracle, rec, tmp_path, min_g):
    """The classes of 8 lanes x 1..4 rows and of 16 lanes x 1..4 rows hold reads that take fewer lanes by default; MGX_PAIRHMM_MIN_G, which
    leads to them, is read once per process, so this test is about a process of its own: it runs pairhmm_f64_cases.py there."""
    path = str(tmp_path / "out.npz")
    env = dict(os.environ, MGX_PAIRHMM_MIN_G=str(min_g), MGX_PAIRHMM_MERGE_BELOW="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pairhmm_f64_cases.py"), str(min_g), path], env=env, check=True, timeout=120)
    z = np.load(path)
    for (G, RPL), g in cases.NEED_MIN_G.items():
        if g != min_g:
            continue
        kernel = cases.kernel_name(G, RPL)
        assert str(z[f"kernel{RPL}"]) == kernel and z[f"used{RPL}"].all() and int(z[f"n_exact{RPL}"]) == 0
        want, _ = cases.fp64_values(oracle, rec, cases.forced_class_batch(G, RPL))
        assert report(kernel, cases.max_diff(z[f"out{RPL}"], want)) < BAR


def test_a_class_of_its_own_at_the_real_threshold(forced, oracle, rec):
    """Without the knob: 4100 test cases of 320 bases are a class of their own, <double, 64, 5>; 64 of them against the recurrence."""
    d, idx = cases.default_threshold_batch()
    check_forced(forced, oracle, rec, d, "pairhmm_fwd<double, 64, 5>", idx)


# ---- b. the strip kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", cases.STRIP_R)
def test_strip_kernel_forced_and_rerun(forced, engine, oracle, rec, R):
    """One row in the second strip (1025), exactly two strips (2048), two strips and a row (2049): forced, and unforced, where the planted
    mismatches send every test case to the strip class's re-run list.  The same bytes both ways."""
    d = cases.strip_batch(R)
    out = check_forced(forced, oracle, rec, d, "pairhmm_fwd_strip<double>")
    out2, used2, st2 = run(engine, d)
    assert used2.all() and st2["n_rerun_f64"] == d["n_pairs"] and st2["n_exact"] == 0
    assert out2.tobytes() == out.tobytes()


# ---- c. the re-run lists as the product uses them ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", cases.RERUN_SHARED + cases.RERUN_OWN16 + cases.RERUN_OWN64)
def test_rerun_lists_of_the_default_engine(engine, oracle, monkeypatch, R):
    """A quarter of the batch stays fp32, the rest goes to the re-run list: the shared narrow one (reads of up to 128 bases; 16 lanes x
    1, 1, 2, 2, 4, 7, 8 rows), a 16-lane class's own (64 x 3) or a 64-lane class's own (64 x 4, 7, 16).  Then without the knob: folded into
    another class, another fp64 shape, the same bytes."""
    d, meant = cases.rerun_batch(R, cases.RERUN_N, 0xCC00 + R)
    want, wused = oracle.batch(d)          # the oracle's own decision: the fp64 recurrence where wused
    assert np.array_equal(wused == 1, meant)
    monkeypatch.setenv(KNOB, "1")
    out, used, st = run(engine, d)
    monkeypatch.delenv(KNOB)
    assert np.array_equal(used, wused) and st["n_rerun_f64"] == int(used.sum()) and st["n_exact"] == 0
    diff = report("re-run list, R = %d, %s" % (R, cases.kernel_name(*cases.RERUN_EXPECT[R])), cases.max_diff(out[meant], want[meant]))
    assert diff < BAR
    assert cases.max_diff(out[~meant], want[~meant]) <= TOL
    out2, used2, st2 = run(engine, d)
    assert np.array_equal(used2, wused) and st2["n_rerun_f64"] == int(used.sum()) and st2["n_exact"] == 0
    assert out2[meant].tobytes() == out[meant].tobytes()
    assert cases.max_diff(out2[~meant], want[~meant]) <= TOL


# ---- d. lists longer than one pass of their grid -------------------------------------------------------------------------------------------

def check_wrap(engine, oracle, d, what):
    want, wused = oracle.batch(d)
    assert wused.all()
    out, used, st = run(engine, d)
    assert used.all() and st["n_rerun_f64"] == d["n_pairs"] and st["n_exact"] == 0
    assert report(what, cases.max_diff(out, want)) < BAR


def test_shared_list_longer_than_its_grid(engine, oracle, n_cu):
    check_wrap(engine, oracle, cases.wrap_shared(n_cu), "shared list of %d, 32 n_cu + 37" % (32 * n_cu + 37))


def test_own_list_of_a_64_lane_class_longer_than_its_grid(engine, oracle, n_cu):
    check_wrap(engine, oracle, cases.wrap_own64(n_cu), "64-lane list of %d, 8 n_cu + 5" % (8 * n_cu + 5))


def test_strip_lists_longer_than_their_grid(engine, oracle, n_cu):
    """4 n_cu + 3 strip test cases: the fp32 launch and the re-run both walk the list with 4 n_cu workgroups, whose boundary scratch is
    indexed by workgroup and used again on the second pass"""
    check_wrap(engine, oracle, cases.wrap_strip(n_cu), "strip list of %d, 4 n_cu + 3" % (4 * n_cu + 3))


def test_exact_tier_list_longer_than_its_grid(engine, oracle, n_cu):
    """flush_regime_pairs through the exact tier, against oracle.batch as test_results_near_the_flush_to_zero_threshold does: the exact tier
    repeats the reference's operation order under flush-to-zero, which is what that oracle computes"""
    from test_pairhmm_oracle import assert_log10_close
    d = cases.wrap_exact(n_cu)
    n = len(d["pair_read"])
    want, _ = oracle.batch(d)
    fin = np.isfinite(want)
    out, used, st = run(engine, d)
    assert used.all()
    assert st["n_exact"] > 2 * n_cu and st["n_exact"] >= int((~fin).sum()) + int((want[fin] < -590).sum())
    assert_log10_close(out, want)
    print("exact tier: %d of %d test cases, grid %d" % (st["n_exact"], n, 2 * n_cu))


# ---- e. a value does not depend on shape or path ---------------------------------------------------------------------------------------------

def test_value_does_not_depend_on_shape_or_path(pkg, forced, engine, oracle, monkeypatch):
    """64 underflowing test cases of 8 .. 128 bases (gcp >= 1, no N: the plain form is chosen per wavefront) computed seven ways give the
    same 8 bytes each.  The shapes each way takes: test_pairhmm_f64_host.py::test_shape_independence_ways."""
    d = cases.shape_independence_batch()
    n = d["n_pairs"]
    want, wused = oracle.batch(d)
    assert wused.all()
    ways = {}
    monkeypatch.setenv(KNOB, "1")
    ways["forced, own classes"] = run(forced, d)[0]
    ways["one by one, the shared launch sized by the read's own rows"] = np.array([run(engine, cases.subset(d, [i]))[0][0] for i in range(n)])
    ways["next to 16 reads of 128 bases, the shared launch of 16 x 8"] = run(engine, cases.concat([d, cases.rerun_part(128, 16, 0xE128)]))[0][:n]
    monkeypatch.delenv(KNOB)
    ways["forced, folded"] = run(forced, d)[0]
    ways["together, folded"] = run(engine, d)[0]
    ways["next to reads of 150 bases, folded"] = run(engine, cases.concat([d, cases.rerun_part(150, 16, 0xE150)]))[0][:n]
    q = pkg.PairHMMQueue(devices=(0,), lanes_per_device=2, batch_pairs=7)
    ways["queue, batches of 7"] = q.run(d)
    q.close()
    first = ways["forced, own classes"]
    assert report("seven ways", cases.max_diff(first, want)) < BAR
    for name, out in ways.items():
        assert out.tobytes() == first.tobytes(), (name, np.flatnonzero(out != first))


# ---- f. content the fp64 emission compares for itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", cases.CONTENT_R)
def test_content_the_fp64_emission_compares_for_itself(forced, engine, oracle, rec, monkeypatch, R):
    """N at the first, last and a middle position of read and haplotype, lower-case and other non-ACGTN bytes, quality bytes of 128 and above in
    all four fields, a row with gap-continuation byte 0 and one with 128 (the fp64 plain form), a row with ins = del = 0: forced, in the
    shape named by CONTENT_KERNEL, and through the re-run list."""
    d = cases.content_batch(R)
    monkeypatch.setenv(KNOB, "1")
    check_forced(forced, oracle, rec, d, cases.CONTENT_KERNEL[R])
    want, wused = oracle.batch(d)
    assert wused.all()
    out, used, st = run(engine, d)
    assert used.all() and st["n_rerun_f64"] == d["n_pairs"] and st["n_exact"] == 0
    assert report("content through the re-run list, R = %d" % R, cases.max_diff(out, want)) < BAR
