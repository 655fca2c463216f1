"""GPU tests of the fp32 PairHMM kernels' emission-table layout (csrc/pairhmm_etab.h): quad tables read 16 bytes at a
time in the classes of 4, 8, 12 and 16 rows per lane, pair tables in the others.  Every read pattern of the column loop is reached through the
kernel of a class of its own and checked against the oracle: the project's 1e-5 on log10 and the oracle's fp64 decisions.

Batch sizes.  64 test cases per shape are checked against the oracle.  The host folds a read-length class of fewer than 4096 test
cases into the widest class of its lane-group width (4 x 8, 8 x 8, 16 x 12, 64 x 16 rows), so 64 test cases alone only ever reach
those four kernels; to run the kernel of their own class they are followed by 4036 more of the same shape, which the device computes
and nobody checks (`dominant_kernel` shows the class was reached).  The 64 are then run once more on their own, which takes them
through the widest class of their width -- another table layout -- and must give the same bytes.
Reads of up to 64 bases go to the 4- and 8-lane classes, so 1 to 4 rows per lane (pair tables only, one quad) are reached there, not
in the 16-lane class; the body and the layout are the same.  The strip-mined class is never folded: 64 test cases, no filler.
Haplotypes of max(R, 2 G) to 48 bases more: fill and drain of G - 1 steps, the unguarded two-column loop and, since the groups of a
wavefront differ in length, the guarded tail all run.  No shorter: a read much longer than its haplotype underflows fp32, and the
fp64 re-run, which has no table, would then be what the oracle is compared with."""
import numpy as np
import pytest

from test_pairhmm_nhap_gpu import THRESHOLD, has_n, put_n, run
from test_pairhmm_oracle import TOL, assert_log10_close

pytestmark = pytest.mark.gpu

CHECKED, BATCH = 64, 4100                    # BATCH: past the 4096 of the folding rule, no multiple of the 4 groups of a workgroup
# (G, RPL, read length): the column loop's reads in that class.  Quad tables where RPL is a multiple of 4, pair tables elsewhere.
SHAPES = [
    (4, 1, 4),        # one pair table, one row: ds_read_b32
    (4, 2, 8),        # one pair table
    (4, 3, 12),       # two pair tables
    (4, 4, 16),       # one quad
    (4, 7, 28),       # four pair tables, the last of one row
    (8, 5, 40),       # three pair tables
    (8, 8, 64),       # two quads
    (16, 5, 80), (16, 6, 96), (16, 7, 112), (16, 8, 128), (16, 9, 144), (16, 10, 160), (16, 12, 192),
    (64, 4, 256),     # one quad, the six-operation cell
    (64, 7, 448),
    (64, 12, 768),    # three quads
    (64, 13, 800),
]


def h_range(G, R):
    return (max(R, 2 * G), max(R, 2 * G) + 48)


def first(d, n):
    return dict(d, pair_read=d["pair_read"][:n], pair_hap=d["pair_hap"][:n])


def concat(parts):
    """Pair-list batches (pair i = read i x haplotype i) one after the other."""
    join = lambda key: np.concatenate([p[key] for p in parts])  # noqa: E731
    offs = lambda key: np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[key].astype(np.int64)) for p in parts]))]).astype(np.uint64)  # noqa: E731
    n = sum(len(p["pair_read"]) for p in parts)
    return dict(n_reads=n, n_haps=n, n_pairs=n, read_off=offs("read_off"), hap_off=offs("hap_off"), bases=join("bases"), qual=join("qual"),
                ins=join("ins"), dele=join("dele"), gcp=join("gcp"), hap_bases=join("hap_bases"),
                pair_read=np.arange(n, dtype=np.uint32), pair_hap=np.arange(n, dtype=np.uint32))


@pytest.fixture(scope="module")
def batches(synth):
    """One batch per (read length, size), made once and left unchanged."""
    made = {}

    def get(G, R, n=BATCH):
        if (R, n) not in made:
            made[(R, n)] = synth.gen_pairhmm_pairs(n, 0xE7AB + R, r_range=(R, R), h_range=h_range(G, R))
        return made[(R, n)]
    return get


@pytest.fixture(scope="module")
def timed(pkg):
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.TIMING)      # the statistics name the launch that did the most work
    yield eng
    eng.close()


def check_against_oracle(oracle, d, out, used):
    want, wused = oracle.batch(d)
    assert_log10_close(out, want)
    clear = np.isinf(want) | (np.abs(want - THRESHOLD) > 2 * TOL)          # float-first: the oracle's decision, away from the threshold
    assert np.array_equal(used[clear], wused[clear])


@pytest.mark.parametrize("G,RPL,R", SHAPES)
def test_every_read_pattern_in_its_own_class(engine, timed, oracle, batches, G, RPL, R):
    d = batches(G, R)
    H = np.diff(d["hap_off"].astype(np.int64))
    assert H.min() >= 2 * G and len(set(H[:CHECKED].tolist())) > 8
    out, used, st = run(timed, d)
    assert (used[:CHECKED] == 0).sum() > CHECKED // 2                       # fp32 results: what the table feeds
    assert st["dominant_kernel"] == f"pairhmm_fwd<float, {G}, {RPL}>"
    sub = first(d, CHECKED)
    check_against_oracle(oracle, sub, out[:CHECKED], used[:CHECKED])
    alone, aused, _ = run(engine, sub)                                     # folded into the widest class of the width: another layout
    assert alone.tobytes() == out[:CHECKED].tobytes() and np.array_equal(aused, used[:CHECKED])


def test_strip_mined_class(engine, oracle, batches):
    d = batches(64, 1100, CHECKED)                                         # 64 lanes x 16 rows per strip, five codes: four quads per column
    out, used, _ = run(engine, d)
    check_against_oracle(oracle, d, out, used)


@pytest.mark.parametrize("G,RPL,R", [(16, 7, 112), (16, 8, 128), (8, 5, 40), (64, 13, 800)])
def test_five_code_table(engine, oracle, batches, G, RPL, R):
    """A quarter of the haplotypes hold an N: those test cases are computed by the class's second launch, from the five-code table
    (same layout as the first launch, five code columns: another size and other table offsets)."""
    d0 = batches(G, R)
    d = put_n(d0, list(range(0, BATCH, 4)))
    out, used, st = run(engine, d)
    assert st["n_nhap_f32"] == int(has_n(d).sum()) == (BATCH + 3) // 4
    check_against_oracle(oracle, first(d, CHECKED), out[:CHECKED], used[:CHECKED])
    plain, pused, _ = run(engine, d0)                                      # the test cases without an N: the same bytes as without the Ns around
    keep = ~has_n(d)
    assert plain[keep].tobytes() == out[keep].tobytes() and np.array_equal(pused[keep], used[keep])


def test_multi_class_launch_against_own_launches(timed, batches):
    """Two 16-lane classes of 4100 test cases (7 and 8 rows per lane) in one batch share pairhmm_fwd_multi<0>, and two narrow ones
    (4 x 7, 8 x 5) pairhmm_fwd_multi<1>; each class alone has a launch of its own (test_every_read_pattern_in_its_own_class
    asserts that).  The same bytes both ways."""
    shapes = [(16, 112), (16, 128), (4, 28), (8, 40)]
    own = [run(timed, batches(G, R)) for G, R in shapes]
    assert all(st["dominant_kernel"].startswith("pairhmm_fwd<float") for _, _, st in own)
    out, used, st = run(timed, concat([batches(G, R) for G, R in shapes]))
    assert st["dominant_kernel"] == "pairhmm_fwd_multi<0>"
    assert out.tobytes() == np.concatenate([o for o, _, _ in own]).tobytes()
    assert np.array_equal(used, np.concatenate([u for _, u, _ in own]))
