"""GPU tests of the two-launch fp32 PairHMM: the first launch of a class has a four-code emission table
and writes no result for a test case whose haplotype holds an N; that test case goes to the class's N-haplotype list
and is computed by the five-code fp32 launch of the same class.  Values, float-first flags and the bits of a test case
must not depend on which of the two launches computed it.

Batch sizes: the host folds a read-length class of fewer than 4096 test cases into the widest class of its lane-group
width, so a small batch only ever reaches the kernels of 4 x 8, 8 x 8, 16 x 12 and 64 x 16 rows.  The batches that are
to run the 7-, 8- and 10-row kernels of 16 lanes (reads of 100, 128 and 151 bases) therefore hold a little over 4096
test cases; the others hold 40.  For the large ones the "alone" check is made on a sample that holds N and N-free
test cases, for the small ones on every test case."""
import numpy as np
import pytest

from test_pairhmm_oracle import TOL, assert_log10_close

pytestmark = pytest.mark.gpu

N = np.uint8(ord("N"))
SMALL, LARGE = 40, 4100                      # LARGE: not a multiple of the 4 groups of a workgroup
SIZES = {20: SMALL, 50: SMALL, 100: LARGE, 128: LARGE, 151: LARGE, 300: SMALL}
KERNEL = {100: "pairhmm_fwd<float, 16, 7>", 128: "pairhmm_fwd<float, 16, 8>", 151: "pairhmm_fwd<float, 16, 10>",
          300: "pairhmm_fwd<float, 64, 16>"}
# log10 of the float-first threshold as the results are scaled: 1e-28f against INITIAL = 2^120
THRESHOLD = -28.0 - 120.0 * np.log10(2.0)


def n_positions(H):
    """Where an N can go wrong in the dword staging: the byte-wise head and tail, and the middle."""
    return [0, 1, 2, 3, H - 1, H - 2, H - 3, H - 4, H // 2]


def put_n(d, which):
    """d with one N in the haplotype of every test case in `which`; the position cycles through n_positions."""
    hap = d["hap_bases"].copy()
    ho = d["hap_off"].astype(np.int64)
    for k, i in enumerate(which):
        H = int(ho[i + 1] - ho[i])
        pos = n_positions(H)
        hap[ho[i] + pos[k % len(pos)]] = N
    return dict(d, hap_bases=hap)


def has_n(d):
    ho = d["hap_off"].astype(np.int64)
    isn = np.concatenate([[0], np.cumsum(d["hap_bases"] == N)])
    return (isn[ho[1:]] - isn[ho[:-1]])[d["pair_hap"]] > 0


def mix(n, name):
    if name == "none":
        return []
    if name == "all":
        return list(range(n))
    if name == "one":
        return [n // 2 + 1]
    return [3, 9, 17, n // 2, n - 1][:5]          # "five": a list that fills no workgroup of any class evenly


def run(engine, d):
    b = engine.batch(d)
    b.run()
    out, used = b.results(with_flags=True)
    st = b.stats()
    b.close()
    return out, used, st


def check(engine, oracle, d, alone):
    """Values and flags against the oracle, the counters, and the test cases `alone` one by one against the batch."""
    want, wused = oracle.batch(d)
    out, used, st = run(engine, d)
    assert_log10_close(out, want)
    # float-first: the same decision as the oracle, except where its value is within the value tolerance of the threshold
    clear = np.isinf(want) | (np.abs(want - THRESHOLD) > 2 * TOL)
    assert np.array_equal(used[clear], wused[clear])
    assert st["n_nhap_f32"] == int(has_n(d).sum())
    assert st["n_rerun_f64"] == int(used.sum())
    for i in alone:
        sub = dict(d, pair_read=d["pair_read"][i:i + 1], pair_hap=d["pair_hap"][i:i + 1])
        o1, u1, _ = run(engine, sub)
        assert o1[0].tobytes() == out[i].tobytes() and u1[0] == used[i], i
    return out, used, want, wused


def sample(n, which):
    if n <= SMALL:
        return range(n)
    near = [i + 1 for i in which[:8] if i + 1 < n]
    return sorted(set(list(which[:9]) + near + [0, 1, 2, n - 1]))


@pytest.fixture(scope="module")
def base(synth):
    """One N-free batch per read length, made once; haplotypes of 40-300 bases, most of them no multiple of 4."""
    made = {}

    def get(R):
        if R not in made:
            made[R] = synth.gen_pairhmm_pairs(SIZES[R], 0xA5A5 + R, r_range=(R, R), h_range=(40, 300))
        return made[R]
    return get


@pytest.fixture(scope="module")
def timed(pkg):
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.TIMING)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", ["none", "all", "one", "five"])
@pytest.mark.parametrize("R", [20, 50, 100, 128, 151, 300])
def test_n_haplotypes_per_class(engine, oracle, base, R, name):
    d0 = base(R)
    n = SIZES[R]
    assert (np.diff(d0["hap_off"].astype(np.int64)) % 4 != 0).sum() > n // 2
    which = mix(n, name)
    d = put_n(d0, which)
    check(engine, oracle, d, sample(n, which))


@pytest.mark.parametrize("R", [100, 128, 151, 300])
def test_batches_reach_the_class_they_are_meant_for(timed, base, R):
    _, _, st = run(timed, put_n(base(R), mix(SIZES[R], "five")))
    assert st["dominant_kernel"] == KERNEL[R]
    assert st["n_nhap_f32"] == 5


def test_mixed_lengths_through_both_multi_class_launches(engine, oracle, synth):
    """Two 16-lane classes (7 and 8 rows per lane) of 4100 test cases each and two narrow ones (reads of 20 and 50
    bases) of 40: small enough to share the two multi-class launches; every class keeps a list of its own."""
    parts = [synth.gen_pairhmm_pairs(k, 0xB0B + R, r_range=(R, R), h_range=(40, 90)) for R, k in
             ((100, LARGE), (128, LARGE), (20, SMALL), (50, SMALL))]
    cat = lambda key: np.concatenate([p[key] for p in parts])  # noqa: E731
    offs = lambda key: np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[key].astype(np.int64)) for p in parts]))]).astype(np.uint64)  # noqa: E731
    n = sum(len(p["pair_read"]) for p in parts)
    d = dict(n_reads=n, n_haps=n, n_pairs=n, read_off=offs("read_off"), hap_off=offs("hap_off"),
             bases=cat("bases"), qual=cat("qual"), ins=cat("ins"), dele=cat("dele"), gcp=cat("gcp"), hap_bases=cat("hap_bases"),
             pair_read=np.arange(n, dtype=np.uint32), pair_hap=np.arange(n, dtype=np.uint32))
    starts = np.cumsum([0] + [len(p["pair_read"]) for p in parts])
    which = sorted(int(s) + k for s in starts[:4] for k in (0, 5, 6, 7, 8, 21, 30, 33, 39))   # 9 per class, every position
    d = put_n(d, which)
    check(engine, oracle, d, which + [w + 1 for w in which if w + 1 < n])


def test_n_haplotype_that_underflows_ends_in_fp64(engine, oracle, synth):
    """Random reads (every base a likely mismatch) drive the fp32 likelihood below 1e-28f: with an N in the haplotype the
    five-code fp32 launch is the one that finds that out and passes the test case on; the others stay float."""
    n = LARGE
    d = synth.gen_pairhmm_pairs(n, 0xF10A7, r_range=(128, 128), h_range=(40, 300), random_read_rate=0.25)
    which = list(range(0, n, 2))
    d = put_n(d, which)
    out, used, want, wused = check(engine, oracle, d, sample(n, which))
    isn = has_n(d)
    far = np.isinf(want) | (np.abs(want - THRESHOLD) > 1.0)
    assert (isn & far & (wused == 1)).sum() > 100 and (isn & far & (wused == 0)).sum() > 100
    assert np.array_equal(used[isn & far], wused[isn & far])
    both = isn & (used == 1) & ~np.isinf(want)
    assert np.abs(out[both] - want[both]).max() < 1e-9          # the fp64 value, not a float one


@pytest.mark.parametrize("R", [50, 128])
def test_plain_form_against_an_n_haplotype(engine, oracle, base, R):
    """A gap-continuation byte 0 makes the wavefront take the plain form of the cell, in the first launch (the N-free
    neighbours) and in the five-code one.  The form is chosen per wavefront, so a neighbour of such a read has other last
    bits than it has alone, with or without this change; the "alone" check is made on the reads that hold the byte 0
    themselves (two against an N haplotype, two not), which take the plain form wherever they are."""
    n = SIZES[R]
    which = mix(n, "five")
    d = put_n(base(R), which)
    gcp = d["gcp"].copy()
    ro = d["read_off"].astype(np.int64)
    zero = (which[0], which[2], which[2] + 1, 0)
    for i in zero:
        gcp[ro[i] + (i % R)] = 0
    d = dict(d, gcp=gcp)
    check(engine, oracle, d, zero)
