"""The five compute contexts (PairHMM, sort / mark-duplicate, Smith-Waterman, activity, BGZF) through create, use and destroy:
the device ordinal each create takes, create / one call / destroy repeated, arrays that grow between calls and are used small
again, the sort context's streamed upload that grows with records in place, the PairHMM strip scratch, and the flagged
streams.  Every comparison is against a fresh context given the same input."""
import ctypes
import errno

import numpy as np
import pytest

from test_pairhmm_oracle import assert_log10_close

pytestmark = pytest.mark.gpu

L_SORT = 200_000        # two contigs of 100 000: a bitmap of 100 KB, not the default's gigabyte


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=np.asarray(x).dtype.kind == "f") for x, y in zip(a, b))


# ---- the smallest input of every kind, and what one call on a context gives for it, as a tuple of arrays ----
def hmm_input(synth):
    return synth.gen_pairhmm_pairs(1, 11, r_range=(10, 10), h_range=(12, 12))


def sort_records(synth, n, seed=3):
    recs, L = synth.gen_sortdedup_packed(n, seed, n_contigs=2, contig_len=L_SORT // 2)
    assert L == L_SORT and len(recs) == n
    return recs


def sort_smallest(synth):
    """one pair plus one fragment"""
    recs = np.concatenate([sort_records(synth, 2), sort_records(synth, 2, seed=4)[:1]])
    recs["mate"][2] = synth.NO_MATE
    recs["flag"][2] = 1 | 8 | 64
    return recs


def sw_input(synth, n, seed=5):
    return synth.gen_sw_pairs(n, seed, ref_range=(8, 8), alt_range=(8, 8)) if n == 1 else synth.gen_sw_pairs(n, seed)


def act_smallest(synth):
    return synth.pack_activity_reads(100, b"A", [dict(start=100, cigar="1M", bases=b"C", quals=[30])])


def hmm_call(e, d):
    return (e.compute(d),)


def sort_call(e, recs):
    return e.sort_mark(L_SORT, recs)


def sw_call(e, w):
    cig, off, score = e.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
    return np.array(cig, dtype=object), off, score


def act_call(e, d):
    return e.interval(d) + (e.last_elements(),)


def bgzf_call(e, data):
    return e.compress(data)


KINDS = ["pairhmm", "sortdedup", "sw", "activity", "bgzf"]


@pytest.fixture(scope="module")
def kinds(pkg, synth):
    """per kind: the create's symbol, the Python engine, its call and its smallest input"""
    return {"pairhmm": ("mgx_pairhmm_create", pkg.PairHMMEngine, hmm_call, hmm_input(synth)),
            "sortdedup": ("mgx_sortdedup_create", pkg.SortDedupEngine, sort_call, sort_smallest(synth)),
            "sw": ("mgx_sw_create", pkg.SmithWatermanEngine, sw_call, sw_input(synth, 1)),
            "activity": ("mgx_activity_create", pkg.ActivityEngine, act_call, act_smallest(synth)),
            "bgzf": ("mgx_bgzf_create", pkg.BgzfCompressor, bgzf_call, b"A")}


def fresh(kinds, kind, data, *args):
    _, engine, call, _ = kinds[kind]
    e = engine(0, *args)
    try:
        return call(e, data)
    finally:
        e.close()


# ---- the device ordinal ----
@pytest.mark.parametrize("kind", KINDS)
def test_device_ordinals(pkg, kinds, kind):
    """An ordinal equal to the device count is -EINVAL and leaves no context.  -1 is taken by every create (round-robin for PairHMM
    and sort contexts, device 0 for the others); any other negative ordinal is -EINVAL, except for BGZF, where it means device 0."""
    import torch
    symbol, engine, call, smallest = kinds[kind]
    lib = pkg.native.load()
    n_dev = torch.cuda.device_count()
    out = ctypes.c_void_p(0xDEAD)
    assert getattr(lib, symbol)(n_dev, 0, ctypes.byref(out)) == -errno.EINVAL
    assert out.value is None
    assert ("device %d out of range (0..%d)" % (n_dev, n_dev - 1)) in lib.mgx_last_error().decode()
    want = fresh(kinds, kind, smallest)
    for device in (-1, -1, -7):      # two draws: with one device both land on it, with more the second lands on the next
        if device == -7 and kind != "bgzf":
            out = ctypes.c_void_p(0xDEAD)
            assert getattr(lib, symbol)(device, 0, ctypes.byref(out)) == -errno.EINVAL and out.value is None
            continue
        e = engine(device)
        assert same(call(e, smallest), want), (kind, device)
        e.close()


@pytest.mark.parametrize("kind", KINDS)
def test_create_call_destroy_three_times(kinds, kind):
    _, _, _, smallest = kinds[kind]
    rounds = [fresh(kinds, kind, smallest) for _ in range(3)]
    assert same(rounds[0], rounds[1]) and same(rounds[0], rounds[2])


# ---- arrays that grow between calls, and are used small again ----
def grow_and_back(kinds, kind, inputs):
    _, engine, call, _ = kinds[kind]
    e = engine(0)
    got = [call(e, d) for d in inputs]
    e.close()
    for d, g in zip(inputs, got):
        assert same(g, fresh(kinds, kind, d)), kind


def test_sortdedup_grows_and_back(kinds, synth):
    """3 records, 10 000 (the work buffers and the staging pair grow), 3"""
    small, large = kinds["sortdedup"][3], sort_records(synth, 10000, seed=7)
    assert len(small) == 3
    grow_and_back(kinds, "sortdedup", [small, large, small])


def test_sw_grows_and_back(kinds, synth):
    grow_and_back(kinds, "sw", [sw_input(synth, 1), sw_input(synth, 300, seed=8), sw_input(synth, 1)])


def test_activity_grows(kinds, synth):
    grow_and_back(kinds, "activity", [kinds["activity"][3], synth.gen_activity_interval(200, 300, 9), kinds["activity"][3]])


def test_sortdedup_streamed_upload_grows_with_records_in_place(pkg, synth):
    """upload_begin expecting one record, then two chunks of 1500: the second grows the record array with the first in it"""
    recs = sort_records(synth, 3000, seed=10)
    e = pkg.SortDedupEngine(0)
    e.upload_chunks(L_SORT, [recs[:1500], recs[1500:]], n_expected=1)
    e.run()
    got = e.results()
    e.close()
    e = pkg.SortDedupEngine(0)
    want = e.sort_mark(L_SORT, recs)
    e.close()
    assert same(got, want) and int(want[1].sum()) > 0


def test_pairhmm_strip_scratch_grows(pkg, synth):
    """A strip-class batch (lengths of test_pairhmm_gpu.py's test_reads_longer_than_one_strip), then one with longer haplotypes
    and more test cases on the same context: the boundary-row scratch grows between the two."""
    first = synth.gen_pairhmm_pairs(4, 81, r_range=(1025, 1100), h_range=(900, 1300), random_read_rate=0.1)
    longer = synth.gen_pairhmm_pairs(8, 82, r_range=(2049, 2200), h_range=(2000, 2600), random_read_rate=0.1)
    e = pkg.PairHMMEngine(0)
    got = [e.compute(first), e.compute(longer), e.compute(first)]
    e.close()
    for d, g in zip((first, longer, first), got):
        f = pkg.PairHMMEngine(0)
        want = f.compute(d)
        f.close()
        assert_log10_close(g, want)
    assert np.array_equal(got[0], got[2])


# ---- flagged streams ----
CU_PATTERN = 0x55 << 8      # flags bits 8..15: every other CU
HIGH_PRIORITY = 1 << 16     # MGX_STREAM_HIGH_PRIORITY


@pytest.mark.parametrize("kind,flags", [("pairhmm", CU_PATTERN), ("sortdedup", CU_PATTERN), ("sortdedup", HIGH_PRIORITY), ("sortdedup", CU_PATTERN | HIGH_PRIORITY)])
def test_flagged_streams(kinds, kind, flags):
    smallest = kinds[kind][3]
    assert same(fresh(kinds, kind, smallest, flags), fresh(kinds, kind, smallest))
