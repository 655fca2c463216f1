"""Row F2 on the CPU: the oracle's read model and normalisation / filter (oracle/pairhmm_oracle.c) against the reference's own
compiled repeat search (tests/golden/read_model.npz, and live where oracle/_ref/ref_read_model is built) and against the Python
restatement of tests/read_model_cases.py, on the cases the device is then held to (tests/test_read_model_gpu.py).  Also what those
cases must satisfy so that no comparison needs a mask: margins from every threshold and cap, and coverage of the seams."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import read_model_cases as C
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "read_model.npz")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "ref_read_model")
MARGIN = 0.5


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def oracle_model(oracle, d, mapq, model):
    """ph_oracle_read_model on a region's reads -> dict of the four modified arrays"""
    m = {k: np.ascontiguousarray(d[k]).copy() for k in ("qual", "ins", "dele", "gcp")}
    ro = np.ascontiguousarray(d["read_off"], dtype=np.uint64)
    oracle.lib.ph_oracle_read_model(ctypes.c_int64(len(ro) - 1), P(ro), P(np.ascontiguousarray(d["bases"])), P(m["qual"]), P(m["ins"]), P(m["dele"]),
                                    P(m["gcp"]), P(np.ascontiguousarray(mapq, dtype=np.uint8)), int(model["pcr_rate_factor"]),
                                    int(model["base_quality_threshold"]), int(model["constant_gcp"]))
    return m


def oracle_normalize_filter(oracle, rows, read_len, log10_rate, max_err):
    """ph_oracle_normalize_filter on [n_reads][n_haps] -> (rows, keep)"""
    io = np.ascontiguousarray(rows, dtype=np.float64).copy()
    ro = np.concatenate([[0], np.cumsum(read_len)]).astype(np.uint64)
    keep = np.zeros(io.shape[0], dtype=np.uint8)
    oracle.lib.ph_oracle_normalize_filter(ctypes.c_int64(io.shape[0]), ctypes.c_int64(io.shape[1]), P(ro), P(io), ctypes.c_double(log10_rate),
                                          ctypes.c_double(max_err), P(keep))
    return io, keep


def own_handle(oracle):
    """a handle of this module's own on the oracle library: argument types set on it are not seen through the shared fixture"""
    return ctypes.CDLL(oracle.lib._name)


_NF_ORACLE = {}


def nf_oracle(oracle, case):
    """The oracle's pipeline on a normalise / filter case, per region: raw (before normalisation), want, keep and the read
    lengths.  Computed once per case and left unchanged."""
    if case["name"] not in _NF_ORACLE:
        per_region = []
        for d, mq in zip(case["plain"], case["mapqs"]):
            n_reads, n_haps = len(d["read_off"]) - 1, len(d["hap_off"]) - 1
            read_len = np.diff(d["read_off"].astype(np.int64))
            if n_reads == 0:
                per_region.append(dict(raw=np.zeros((0, n_haps)), want=np.zeros((0, n_haps)), keep=np.zeros(0, dtype=np.uint8), read_len=read_len))
                continue
            dm = dict(d)
            dm.update(oracle_model(oracle, d, mq, case["model"]))
            raw = oracle.batch(dm)[0].reshape(n_reads, n_haps)
            want, keep = oracle_normalize_filter(oracle, raw, read_len, case["model"]["log10_mismapping_rate"], case["model"]["max_error_per_base"])
            for a in (raw, want, keep):
                a.setflags(write=False)
            per_region.append(dict(raw=raw, want=want, keep=keep, read_len=read_len))
        _NF_ORACLE[case["name"]] = per_region
    return _NF_ORACLE[case["name"]]


def test_golden_file_was_made_for_these_cases(golden):
    assert str(golden["digest"][0]) == C.digest()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert len(golden["reps"]) == C.N_REPS == len(C.reps_triples())
    assert len(golden["rl"]) == sum(len(r["bases"]) for c in C.model_cases() for r in c["reads"])


def test_repetition_counts_equal_the_reference(oracle, golden):
    """findNumberOfRepetitions as the oracle restates it, as the Python restatement does, and as the reference build answered"""
    triples = C.reps_triples()
    lens = [len(u) for u, _, _ in triples]
    assert set(lens) == set(range(1, 10)) and {len(t) for _, t, _ in triples} == set(range(0, 65)) and {lead for _, _, lead in triples} == {0, 1}
    fn = own_handle(oracle).ph_oracle_n_repetitions
    fn.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    fn.restype = ctypes.c_int
    got = np.array([fn(u, len(u), t, len(t), lead) for u, t, lead in triples])
    assert np.array_equal(got, golden["reps"])
    assert np.array_equal(np.array([C.count_repetitions(u, t, lead) for u, t, lead in triples]), golden["reps"])
    assert (golden["reps"] >= 8).sum() > 1000 and (golden["reps"] == 0).sum() > 1000


def test_reference_build_gives_the_golden_answers(golden, tmp_path):
    """live, where the reference build is there: both overloads on the triples, and every case"""
    if not os.path.exists(REF_EXE):
        pytest.skip("oracle/_ref/ref_read_model is not built here (it needs the reference tree); the golden file stands for it")
    path = str(tmp_path / "reps.txt")
    with open(path, "w") as f:
        f.write(C.reps_text(C.reps_triples()))
    pairs = np.array(subprocess.run([REF_EXE, "reps", path], check=True, capture_output=True, text=True).stdout.split(), dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(pairs[:, 0], golden["reps"]) and np.array_equal(pairs[:, 1], golden["reps"])
    path = str(tmp_path / "reads.txt")
    with open(path, "w") as f:
        f.write(C.reads_text(C.model_cases()))
    live = C.parse_reads_answers(subprocess.run([REF_EXE, "reads", path], check=True, capture_output=True, text=True).stdout, C.model_cases())
    assert live == C.golden_answers(golden, C.model_cases())


def test_read_model_oracle_restatement_and_golden_agree(oracle, golden):
    """byte for byte, on every case, every read and every offset: the repeat length (ph_oracle_tandem_repeat), the cache table and
    the four modified arrays (ph_oracle_read_model), from the oracle, the Python restatement and the reference build"""
    cases = C.model_cases()
    want = C.golden_answers(golden, cases)
    restated = C.restated_answers()
    tandem = own_handle(oracle).ph_oracle_tandem_repeat
    tandem.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    tandem.restype = ctypes.c_int
    for c, (w_cache, w_reads), (r_cache, r_reads) in zip(cases, want, restated):
        assert w_cache == r_cache, c["name"]
        d, mapq = C.case_region(c)
        m = oracle_model(oracle, d, mapq, c["model"])
        ro = d["read_off"].astype(np.int64)
        for i, (r, w, rs) in enumerate(zip(c["reads"], w_reads, r_reads)):
            where = (c["name"], i)
            assert rs == w, where
            n = len(r["bases"])
            assert bytes(tandem(r["bases"], n, k) for k in range(n)) == w[0], where
            for key, w_bytes in zip(("qual", "ins", "dele", "gcp"), w[1:]):
                assert m[key][ro[i]:ro[i + 1]].tobytes() == w_bytes, where + (key,)
    # the oracle's cache formula, through its effect: a long homopolymer under ins / del of 255 shows the cache value itself
    for rate in (1, 2, 3):
        for total in range(1, 21):
            b = b"C" + b"A" * total + b"G"
            hi = bytes([255] * len(b))
            got = C.restated_model(b, hi, hi, hi, hi, 60, rate, 18, 10)
            region = dict(read_off=np.array([0, len(b)], dtype=np.uint64), bases=np.frombuffer(b, dtype=np.uint8),
                          **{k: np.frombuffer(hi, dtype=np.uint8) for k in ("qual", "ins", "dele", "gcp")})
            m = oracle_model(oracle, region, [60], dict(pcr_rate_factor=rate, base_quality_threshold=18, constant_gcp=10))
            assert m["ins"].tobytes() == got[1] and m["dele"].tobytes() == got[2]
            assert got[1][1] == C.pcr_cache(rate)[total]


def test_cases_reach_every_seam():
    """every repeat length that can occur is reached (0 cannot: both searches count the unit they start from, so a base's
    repeat length is at least 1), every unit length 1..8 ends a search somewhere, the units-differ branch is taken with the
    backward count zero and non-zero, and the cap of 20 cuts totals above it"""
    seen, decided, differ = set(), set(), set()
    by_case = {}
    for c in C.model_cases():
        for r in c["reads"]:
            for i in range(len(r["bases"])):
                trace = {}
                rl = C.repeat_length(r["bases"], i, trace)
                seen.add(rl)
                decided |= trace.get("decided", set())
                if "differ" in trace:
                    differ.add(min(trace["differ"], 1))
                    by_case.setdefault(c["name"], set()).add(min(trace["differ"], 1))
    assert seen == set(range(1, 21))
    assert decided == set(range(1, 9))
    assert differ == {0, 1} and by_case["units_differ"] == {0, 1}
    assert C.repeat_length(b"TTCTTCCCC", 5) == 4                                   # the reference's own example (:239-240)
    nine = C.UNITS[8] * 2
    assert len(C.UNITS[8]) == 9 and max(C.repeat_length(nine, i) for i in range(len(nine))) == 1      # 9 bases twice are not found
    lens = {len(r["bases"]) for c in C.model_cases() for r in c["reads"]}
    assert {1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 1100} <= lens
    models = {(c["model"]["pcr_rate_factor"], c["model"]["base_quality_threshold"], c["model"]["constant_gcp"]) for c in C.model_cases()}
    assert {m[0] for m in models} == {0, 1, 2, 3} and {m[1] for m in models} == {6, 18} and {m[2] for m in models} == {-1, 0, 10}


def synthetic_rows():
    """rows for the normalise / filter step alone: values around the thresholds and caps, -inf entries, rows of -inf"""
    rng = np.random.RandomState(5)
    out = []
    for n_haps in (1, 2, 3, 64, 65):
        for read_len in (1, 49, 50, 51, 99, 100, 101, 150, 2000):
            rows = -30.0 * rng.rand(12, n_haps)
            rows[0, 0] = -5.6
            rows[0, 1:] = -9.1
            rows[1, :] = -math.inf
            rows[2, rng.randint(n_haps)] = -math.inf
            rows[3, :] = -4.0
            rows[4, :] = -8.0
            rows[5, 0] = np.nextafter(-4.0, -10.0)
            rows[6, 0] = np.nextafter(-8.0, -10.0)
            out.append((rows, [read_len] * len(rows)))
    return out


@pytest.mark.parametrize("log10_rate", [-4.5, -3.0, -math.inf])
@pytest.mark.parametrize("max_err", [0.02, float(np.nextafter(0.02, 1.0)), 0.01, 0.05])
def test_normalize_filter_oracle_equals_restatement(oracle, log10_rate, max_err):
    dropped = kept = 0
    for rows, read_len in synthetic_rows():
        want_rows, want_capped, want_keep = C.restated_normalize_filter(rows, read_len, log10_rate, max_err)
        got_rows, got_keep = oracle_normalize_filter(oracle, rows, read_len, log10_rate, max_err)
        assert not np.isnan(got_rows).any()
        assert got_rows.tobytes() == np.array(want_rows, dtype=np.float64).reshape(got_rows.shape).tobytes()
        assert list(got_keep) == want_keep
        assert np.array_equal(got_rows != rows, np.array(want_capped).reshape(rows.shape))
        dropped += want_keep.count(0); kept += want_keep.count(1)
    assert dropped and kept


def test_normalize_filter_cases_keep_their_distance(oracle):
    """No comparison of tests/test_read_model_gpu.py needs a mask, because every case keeps its distance: every read's best value
    lies at least 0.5 from its threshold, and every haplotype value at least 0.5 from its row's cap (the device and the oracle
    agree to 1e-5).  A case that fails here is to be changed, not the margin."""
    seen_keep, seen_capped, seen_free = set(), 0, 0
    for case in C.nf_cases():
        rate, max_err = case["model"]["log10_mismapping_rate"], case["model"]["max_error_per_base"]
        for g, o in enumerate(nf_oracle(oracle, case)):
            rows, capped, keep = C.restated_normalize_filter(o["raw"], o["read_len"], rate, max_err)
            assert list(o["keep"]) == keep and o["want"].tobytes() == np.array(rows, dtype=np.float64).reshape(o["want"].shape).tobytes()
            for r, row in enumerate(o["raw"]):
                where = (case["name"], g, r)
                best = row.max()
                thr = min(2.0, math.ceil(int(o["read_len"][r]) * max_err)) * -4.0
                assert abs(best - thr) >= MARGIN, where + (best, thr)
                seen_keep.add(keep[r])
                if not math.isinf(rate) and len(row) > 1 and not math.isinf(best):
                    gap = np.abs(row - (best + rate))
                    assert gap.min() >= MARGIN, where + (float(gap.min()),)
                    seen_capped += sum(capped[r]); seen_free += len(row) - 1 - sum(capped[r])
    assert seen_keep == {0, 1} and seen_capped and seen_free


def test_normalize_filter_cases_hold_what_the_seams_need(oracle):
    by_name = {c["name"]: c for c in C.nf_cases()}
    # one Q30 mismatch is dropped up to 50 bases and kept from 51; two are dropped, verbatim is kept everywhere
    for R, one in ((49, 0), (50, 0), (51, 1), (100, 1), (101, 1)):
        assert list(nf_oracle(oracle, by_name["seam_R%d" % R])[0]["keep"]) == [1, one, 0, 1, one, 0]
    assert list(nf_oracle(oracle, by_name["seam_R50_rate_one_ulp_up"])[0]["keep"]) == [1, 1, 0, 1, 1, 0]      # ceil(50 * (0.02 + ulp)) = 2
    # every width holds an entry one mismatch from the best that is not capped, and capped ones (from 3 haplotypes on)
    for n_haps in (2, 63, 64, 65, 128, 129):
        o = nf_oracle(oracle, by_name["width_%d" % n_haps])[0]
        for raw, want in zip(o["raw"], o["want"]):
            assert ((raw == want) & (raw < raw.max())).any()
            assert n_haps == 2 or (raw != want).any()
    o = nf_oracle(oracle, by_name["width_1"])[0]
    assert np.array_equal(o["raw"], o["want"])
    # rows of -inf
    o = nf_oracle(oracle, by_name["all_minus_inf"])[0]
    assert np.isneginf(o["raw"]).all() and np.isneginf(o["want"]).all() and list(o["keep"]) == [0]
    o = nf_oracle(oracle, by_name["one_minus_inf"])[0]
    assert np.isfinite(o["raw"][0, 0]) and np.isneginf(o["raw"][0, 1]) and o["want"][0, 1] == o["raw"][0, 0] - 4.5 and list(o["keep"]) == [1]
    # layout: MAPQs are distinct per read and cap the base qualities, the sub-view does not start at 0
    for name in ("layout_empty", "layout_subview"):
        c = by_name[name]
        mq = np.concatenate(c["mapqs"])
        assert len(set(mq.tolist())) == len(mq) and mq.max() < 40
    assert len(by_name["layout_empty"]["regions"][1]["read_off"]) == 1
    sub = by_name["layout_subview"]["regions"][1]
    assert sub["read_off"][0] > 0 and sub["hap_off"][0] > 0
    assert {c["model"]["log10_mismapping_rate"] for c in C.nf_cases()} == {-4.5, -3.0, -math.inf}
    assert {len(d["read_off"]) - 1 for c in C.nf_cases() for d in c["regions"]} >= {0, 1, 3, 4, 5}
