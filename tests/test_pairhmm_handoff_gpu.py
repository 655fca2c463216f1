"""GPU tests of the five-operation sweep's lane hand-off and last-row sum: a lane's bottom row hands two values to the next
lane, evaluated with that lane's top-row coefficients, and read row R sums its m in its own yb.  Both are the operations of the sweep
before them on the same operand bits, so every result must have the BYTES that sweep gave: tests/golden/pairhmm_handoff_bits.npz holds
out_log10 and used_f64 of every batch of pairhmm_handoff_cases.py as the commit before the change computed them on the device.  Values
are also compared with the oracle, at the tolerance test_pairhmm_fiveop_gpu.py uses (assert_log10_close)."""
import numpy as np
import pytest

import pairhmm_handoff_cases as cases
from test_pairhmm_oracle import assert_log10_close

pytestmark = pytest.mark.gpu

NAMES = [name for name, _, _ in cases.batches(4)]


@pytest.fixture(scope="module")
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope="module")
def bits(engine):
    """every batch of the default lane widths, run once"""
    return cases.as_bits(cases.run_batches(engine, 4), 4)


@pytest.fixture(scope="module")
def by_name():
    return {name: d for name, _, d in cases.batches(4)}


def check(bits, golden, oracle, min_g, name, d):
    key = f"g{min_g}/{name}/"
    out = np.frombuffer(bits[key + "out_log10"].tobytes(), dtype=np.float64)
    used = np.frombuffer(bits[key + "used_f64"].tobytes(), dtype=np.uint8)
    assert len(out) == d["n_pairs"]
    want, _ = oracle.batch(d)
    assert_log10_close(out, want)
    differ = np.flatnonzero(out.view(np.uint64) != np.frombuffer(golden[key + "out_log10"].tobytes(), dtype=np.uint64))
    assert differ.size == 0, (name, [(int(i), int(d["R"][i]), int(d["H"][i])) for i in differ[:8]])
    assert used.tobytes() == golden[key + "used_f64"].tobytes(), name
    # the bytes are the five-operation sweep's own only where the result stayed fp32: every test case but the ones deferred on purpose
    mask = cases.five_mask(name, d) if name != "all_classes_one_batch" else np.ones(len(out), dtype=bool)
    assert not used[mask].any(), (name, np.flatnonzero(mask & (used != 0)))


@pytest.mark.parametrize("name", NAMES)
def test_bytes_of_the_sweep_before_and_oracle(bits, golden, oracle, by_name, name):
    check(bits, golden, oracle, 4, name, by_name[name])


def test_own_launch_and_multi_class_launch_agree(bits):
    """the classes one by one (pairhmm_fwd) and all in one batch (pairhmm_fwd_multi for those of up to 8 rows): the same bytes"""
    own = [n for n in NAMES if n.startswith("own_")]
    for kind in ("out_log10", "used_f64"):
        assert np.concatenate([bits[f"g4/{n}/{kind}"] for n in own]).tobytes() == bits[f"g4/all_classes_one_batch/{kind}"].tobytes()


@pytest.mark.parametrize("min_g", [8, 16])
def test_wider_groups_for_short_reads(golden, oracle, tmp_path, min_g):
    """MGX_PAIRHMM_MIN_G is read once per process, so the 8- and 16-lane classes of 1 and 2 rows, and 1 and 2 lanes in use out of 16, are
    about a process of its own: pairhmm_handoff_cases.py runs there"""
    bits = cases.run_in_own_process(min_g, str(tmp_path / "bits.npz"))
    made = cases.batches(min_g)
    assert sorted(bits) == sorted(k for k in golden.files if k.startswith(f"g{min_g}/")) and len(bits) == 2 * len(made)
    for name, _, d in made:
        check(bits, golden, oracle, min_g, name, d)
