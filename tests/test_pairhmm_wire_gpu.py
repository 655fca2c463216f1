"""GPU tests of the PairHMM wire form (MGX_PAIRHMM_WIRE): the device kernel pairhmm_expand_wire restores byte for byte what the
host reference expander gives, a queue or a context with the flag returns the bits of one without it -- likelihoods and
used_f64 flags -- and fewer bytes cross PCIe, exactly as many as the closed form of csrc/pairhmm_wire.h says."""
import numpy as np
import pytest

import pairhmm_wire_cases as W
from test_queue_cpu import _streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wire_engine(pkg):
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.WIRE)
    yield eng
    eng.close()


def device_expansion_equals_host(pkg, wire_engine, d, what):
    """a batch in pair-list form on the WIRE context: its device-resident arrays against the host expander's"""
    p = pkg.pairhmm.pack_batch(d, 0, d["n_pairs"])          # first-use order: packing it again is the identity
    want = pkg.pairhmm.wire_expand(pkg.pairhmm.pack_batch_wire(p, 0, p["n_pairs"]))
    W.assert_same_batch(want, W.canonical(p), what)
    b = wire_engine.batch(p)
    got = b.read_inputs()
    b.close()
    for k in W.ARRAYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def test_device_expansion_on_the_crafted_cases(pkg, wire_engine):
    for name, d in W.crafted().items():
        device_expansion_equals_host(pkg, wire_engine, d, name)


def test_device_expansion_on_a_ragged_batch(pkg, wire_engine, synth):
    d = synth.gen_pairhmm_pairs(2000, 0x5EED0011, r_range=(1, 130), h_range=(10, 200), hap_n_rate=0.004)
    rng = np.random.RandomState(2)
    for k in ("qual", "ins", "dele"):                          # 7-bit, 6-bit and high-bit bytes side by side
        d[k] = (d[k] | np.where(rng.randint(0, 8, len(d[k])) == 0, 128, 0)).astype(np.uint8)
    d["qual"] = (d["qual"] + np.uint8(30)).astype(np.uint8)
    d["gcp"] = rng.randint(0, 40, len(d["gcp"])).astype(np.uint8)
    device_expansion_equals_host(pkg, wire_engine, d, "ragged")
    # a plain context's arrays are the caller's bytes: read_inputs shows the difference the kernels' mask hides
    p = pkg.pairhmm.pack_batch(d, 0, 2000)
    eng = pkg.PairHMMEngine(0)
    b = eng.batch(p)
    got = b.read_inputs()
    b.close(); eng.close()
    for k in W.ARRAYS:
        assert np.array_equal(got[k], p[k]), k


def plain_results(engine, d):
    b = engine.batch(d)
    b.run()
    out, used = b.results(with_flags=True)
    b.close()
    return out, used


def closed_form_bytes(pkg, d, n, batch_pairs):
    wire = plain = 0
    for lo in range(0, n, batch_pairs):
        hi = min(n, lo + batch_pairs)
        wire += pkg.pairhmm.wire_upload_bytes(pkg.pairhmm.pack_batch_wire(d, lo, hi))
        plain += pkg.pairhmm.plain_upload_bytes(pkg.pairhmm.pack_batch(d, lo, hi))
    return wire, plain


@pytest.mark.parametrize("name", ["region", "cross", "independent", "shuffled"])
def test_wire_queue_returns_the_plain_bits(pkg, engine, synth, name):
    d = _streams(synth)[name]
    full = dict(d)
    if full.get("pair_read") is None:
        nr, nh = len(d["read_off"]) - 1, len(d["hap_off"]) - 1
        full["pair_read"] = np.repeat(np.arange(nr, dtype=np.uint32), nh); full["pair_hap"] = np.tile(np.arange(nh, dtype=np.uint32), nr)
    want, wused = plain_results(engine, full)
    q = pkg.PairHMMQueue(devices=(0,), lanes_per_device=3, depth=2, batch_pairs=50, flags=pkg.pairhmm.WIRE)
    got, used = q.run(d, with_flags=True)
    st = q.stats()
    q.close()
    assert np.array_equal(got, want) and np.array_equal(used, wused)
    wire_bytes, plain_bytes = closed_form_bytes(pkg, d, len(want), 50)
    assert st["bytes_h2d"] == wire_bytes < plain_bytes


@pytest.fixture(scope="module")
def everything(synth):
    return W.ragged_with_everything(synth, zero_gcp_in_short_reads=False)


def differing(a, b):
    return int((a[0] != b[0]).sum()), int((a[1] != b[1]).sum())


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one_device", "two_device_slots"])
def test_wire_queue_on_every_launch_path(pkg, engine, everything, devices):
    """WIRE queue against one call of a plain engine on the whole stream: likelihoods and used_f64 flags, bit for bit"""
    d = everything
    n = len(d["pair_read"])
    b = engine.batch(d)
    b.run()
    want = b.results(with_flags=True)
    st = b.stats()
    b.close()
    # the stream does reach the launches it was built for
    assert st["n_nhap_f32"] > 0 and st["n_rerun_f64"] > 0 and want[1].any() and not want[1].all()
    assert (np.diff(d["read_off"].astype(np.int64)) == 1100).sum() == 1 and (d["gcp"] == 0).any() and (d["qual"] >= 128).any()
    q = pkg.PairHMMQueue(devices=devices, lanes_per_device=2, depth=2, batch_pairs=500, flags=pkg.pairhmm.WIRE)
    got = q.run(d, with_flags=True)
    qs = q.stats()
    plain = pkg.PairHMMQueue(devices=devices, lanes_per_device=2, depth=2, batch_pairs=500)
    pgot = plain.run(d, with_flags=True)
    ps = plain.stats()
    q.close(); plain.close()
    print("differing (log10, used_f64): wire queue / engine", differing(got, want), "plain queue / engine", differing(pgot, want),
          "wire queue / plain queue", differing(got, pgot))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(pgot[0], want[0]) and np.array_equal(pgot[1], want[1])
    # the bytes did shrink, to the closed form
    wire_bytes, plain_bytes = closed_form_bytes(pkg, d, n, 500)
    assert qs["bytes_h2d"] == wire_bytes and ps["bytes_h2d"] == plain_bytes and qs["bytes_h2d"] < ps["bytes_h2d"]
    assert qs["n_batches"] == ps["n_batches"] == (n + 499) // 500


def test_compute_in_pair_list_form_on_a_wire_context(pkg, engine, wire_engine, everything):
    want, wused = plain_results(engine, everything)
    got, used = plain_results(wire_engine, everything)
    assert np.array_equal(got, want) and np.array_equal(used, wused)
    assert np.array_equal(wire_engine.compute(everything), want)


def test_cross_product_and_regions_are_out_of_scope(pkg, engine, wire_engine, synth):
    """the cross-product form and compute_regions upload as without the flag, and return the plain context's bits"""
    region = synth.gen_pairhmm_region(37, 11, 5, r_range=(20, 90), h_range=(40, 120))
    cross = dict(region); cross["pair_read"] = None; cross["pair_hap"] = None
    assert np.array_equal(wire_engine.compute(cross), engine.compute(cross))
    b = wire_engine.batch(cross)
    got = b.read_inputs()                                    # the caller's bytes, not a canonical form
    b.close()
    assert np.array_equal(got["qual"], region["qual"]) and np.array_equal(got["hap_bases"], region["hap_bases"])
    regions = [synth.gen_pairhmm_region(5 + g, 2 + g % 5, 200 + g, r_range=(20, 128), h_range=(64, 256)) for g in range(8)]
    for a, b in zip(wire_engine.compute_regions(regions), engine.compute_regions(regions)):
        assert np.array_equal(a, b)
    q = pkg.PairHMMQueue(devices=(0,), lanes_per_device=2, batch_pairs=300, flags=pkg.pairhmm.WIRE)
    p = pkg.PairHMMQueue(devices=(0,), lanes_per_device=2, batch_pairs=300)
    for a, b in zip(q.run_regions(regions), p.run_regions(regions)):
        assert np.array_equal(a, b)
    assert q.stats()["bytes_h2d"] == p.stats()["bytes_h2d"]
    q.close(); p.close()


@pytest.mark.parametrize("env,flags,expect_wire", [("0", "WIRE", False), ("1", "plain", True)])
def test_environment_overrides_the_flag(pkg, synth, monkeypatch, env, flags, expect_wire):
    d = synth.gen_pairhmm_pairs(600, 0x5EED0012, r_range=(20, 100), h_range=(40, 150))
    wire_bytes, plain_bytes = closed_form_bytes(pkg, d, 600, 200)
    monkeypatch.setenv("MGX_PAIRHMM_WIRE", env)              # read when the context is created
    q = pkg.PairHMMQueue(devices=(0,), lanes_per_device=2, batch_pairs=200, flags=pkg.pairhmm.WIRE if flags == "WIRE" else 0)
    monkeypatch.delenv("MGX_PAIRHMM_WIRE")
    got = q.run(d)
    st = q.stats()
    q.close()
    assert st["bytes_h2d"] == (wire_bytes if expect_wire else plain_bytes) and wire_bytes < plain_bytes
    eng = pkg.PairHMMEngine(0)
    assert np.array_equal(got, eng.compute(d))
    eng.close()
