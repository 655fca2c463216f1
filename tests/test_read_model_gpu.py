"""Row F2 on the device at its seams: the bytes pairhmm_read_model leaves (through the mgx_pairhmm_regions_modified_inputs hook) against
the reference build's answers (tests/golden/read_model.npz) and the Python restatement, and pairhmm_normalize_filter_rows against
the restatement and the oracle pipeline, on the cases of tests/read_model_cases.py.  No entry and no read is masked out of a
comparison: tests/test_read_model_host.py asserts that the cases keep their distance from every threshold and cap."""
import math
import os

import numpy as np
import pytest

import read_model_cases as C
from conftest import ROOT
from test_pairhmm_oracle import assert_log10_close
from test_read_model_host import nf_oracle

pytestmark = pytest.mark.gpu

KEYS = ("qual", "ins", "dele", "gcp")
LONG_HAP = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(3).randint(0, 4, 150)])


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "read_model.npz"))
    assert str(z["digest"][0]) == C.digest()
    return C.golden_answers({k: z[k] for k in z.files}, C.model_cases())


def model_of(case):
    return dict(case["model"])


def check_bytes(case, got, golden_reads, restated_reads):
    """one region's four arrays from the device == golden == restatement, read by read"""
    d, _ = C.case_region(case)
    ro = d["read_off"].astype(np.int64)
    assert all(len(got[k]) == ro[-1] for k in KEYS)
    for i, (w, rs) in enumerate(zip(golden_reads, restated_reads)):
        assert rs == w, (case["name"], i)
        for k, w_bytes in zip(KEYS, w[1:]):
            g = got[k][ro[i]:ro[i + 1]].tobytes()
            if g != w_bytes:
                at = next(j for j in range(len(g)) if g[j] != w_bytes[j])
                raise AssertionError((case["name"], i, k, "offset", at, "of", len(g), "device", g[at], "reference", w_bytes[at]))


@pytest.mark.parametrize("ci", range(len(C.model_cases())), ids=[c["name"] for c in C.model_cases()])
def test_modified_bytes_of_one_case(engine, golden, ci):
    case = C.model_cases()[ci]
    d, mapq = C.case_region(case, LONG_HAP)
    (got,) = engine.regions_modified_inputs([d], [mapq], **model_of(case))
    check_bytes(case, got, golden[ci][1], C.restated_answers()[ci][1])
    # the same bytes feed the recurrence: with normalisation off the region call equals, bit for bit, the plain PairHMM on
    # the golden-modified arrays as an explicit pair list
    dm = dict(d)
    for k, col in zip(KEYS, range(1, 5)):
        dm[k] = np.frombuffer(b"".join(w[col] for w in golden[ci][1]), dtype=np.uint8)
    raw, _ = engine.region(d, mapq, log10_mismapping_rate=-math.inf, **model_of(case))
    assert np.array_equal(raw.ravel(), engine.compute(dm))


def test_modified_bytes_of_all_cases_in_one_call(engine, golden):
    """every case as one region of a call, the cases that share a model together; an empty region in between changes nothing"""
    cases = C.model_cases()
    by_model = {}
    for ci, c in enumerate(cases):
        by_model.setdefault(tuple(sorted(c["model"].items())), []).append(ci)
    assert max(len(v) for v in by_model.values()) >= 6
    for key, members in by_model.items():
        regions, mapqs = [], []
        for ci in members:
            d, mq = C.case_region(cases[ci], LONG_HAP)
            regions.append(d); mapqs.append(mq)
        empty = dict(regions[0], read_off=np.zeros(1, dtype=np.uint64))
        regions.insert(1, empty); mapqs.insert(1, np.zeros(0, dtype=np.uint8))
        got = engine.regions_modified_inputs(regions, mapqs, **dict(key))
        assert all(len(got[1][k]) == 0 for k in KEYS)
        del got[1]
        for ci, g in zip(members, got):
            check_bytes(cases[ci], g, golden[ci][1], C.restated_answers()[ci][1])


def test_hook_without_test_cases_writes_nothing(engine, golden):
    case = C.model_cases()[0]
    d, mq = C.case_region(case)
    no_haps = dict(d, hap_off=np.zeros(1, dtype=np.uint64))
    (got,) = engine.regions_modified_inputs([no_haps], [mq])
    assert all(not got[k].any() for k in KEYS)                  # the veneer's zero-filled arrays, untouched
    assert engine.regions_modified_inputs([], []) == []
    # in a call that has test cases, a region with reads and no haplotypes is staged, modified and copied back like any other
    got = engine.regions_modified_inputs([no_haps, d], [mq, mq], **model_of(case))
    for g in got:
        check_bytes(case, g, golden[0][1], C.restated_answers()[0][1])


def device_nf(engine, case):
    """per region (raw, got, keep): the device's values with normalisation off, and the whole call"""
    model = dict(case["model"])
    off = dict(model, log10_mismapping_rate=-math.inf)
    raws = engine.regions(case["regions"], case["mapqs"], **off)
    gots = engine.regions(case["regions"], case["mapqs"], **model)
    return [(rw, o, k) for (rw, _), (o, k) in zip(raws, gots)]


@pytest.mark.parametrize("ni", range(len(C.nf_cases())), ids=[c["name"] for c in C.nf_cases()])
def test_normalize_filter_case(engine, oracle, ni):
    case = C.nf_cases()[ni]
    rate, max_err = case["model"]["log10_mismapping_rate"], case["model"]["max_error_per_base"]
    for g, ((raw, got, keep), o) in enumerate(zip(device_nf(engine, case), nf_oracle(oracle, case))):
        assert raw.shape == o["raw"].shape and got.shape == o["want"].shape
        assert not np.isnan(got).any()
        assert_log10_close(raw.ravel(), o["raw"].ravel())
        assert_log10_close(got.ravel(), o["want"].ravel())
        # on the device's own doubles: every capped entry is its row's maximum + rate, every other entry is untouched
        rows, capped, _ = C.restated_normalize_filter(raw, o["read_len"], rate, max_err)
        assert got.tobytes() == np.array(rows, dtype=np.float64).reshape(got.shape).tobytes(), (case["name"], g)
        # the capped set and the keep decision are the oracle pipeline's, for every entry and every read
        _, capped_want, keep_want = C.restated_normalize_filter(o["raw"], o["read_len"], rate, max_err)
        assert capped == capped_want, (case["name"], g)
        assert list(keep) == keep_want == list(o["keep"]), (case["name"], g)
        # and what one region call returns
        d, mq = case["regions"][g], case["mapqs"][g]
        one, one_keep = engine.region(d, mq, **case["model"])
        assert one.tobytes() == got.tobytes() and np.array_equal(one_keep, keep), (case["name"], g)


def test_realign_regions_return_the_same_values(pkg, engine, sw_engine):
    case = next(c for c in C.nf_cases() if c["name"] == "layout_subview")
    res = pkg.RealignEngine(engine, sw_engine).regions(case["regions"], case["mapqs"], **case["model"])
    for o, (_, got, keep) in zip(res, device_nf(engine, case)):
        assert o["log10"].tobytes() == got.tobytes() and np.array_equal(o["keep"], keep)
