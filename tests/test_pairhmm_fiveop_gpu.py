"""GPU tests of the five-operation fp32 PairHMM cell: the first fp32 launch of the classes of up to 16 lanes
(reads of at most 192 bases).  A test case the form cannot take -- a read row with matchToMatchProb 0 or a gap-continuation
byte 0, or a result that is not finite -- joins its class's N-haplotype list and is computed by the second launch; which
launch computed a test case, what else is in the batch and whether its class ran alone or in a multi-class launch must
not show in its bytes."""
import numpy as np
import pytest

from pairhmm_fiveop_cases import DYNAMIC, STATIC, emulate, has_n, overflowing_pair, whole_quality_range, with_qualities
from test_pairhmm_nhap_gpu import check, run
from test_pairhmm_oracle import assert_log10_close

pytestmark = pytest.mark.gpu


def cat(parts):
    """Pair-list batches one after the other."""
    join = lambda key: np.concatenate([p[key] for p in parts])  # noqa: E731
    offs = lambda key: np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[key].astype(np.int64)) for p in parts]))]).astype(np.uint64)  # noqa: E731
    nr, nh = np.cumsum([0] + [len(p["read_off"]) - 1 for p in parts]), np.cumsum([0] + [len(p["hap_off"]) - 1 for p in parts])
    return dict(n_reads=int(nr[-1]), n_haps=int(nh[-1]), n_pairs=sum(len(p["pair_read"]) for p in parts),
                read_off=offs("read_off"), hap_off=offs("hap_off"), bases=join("bases"), qual=join("qual"), ins=join("ins"), dele=join("dele"),
                gcp=join("gcp"), hap_bases=join("hap_bases"),
                pair_read=np.concatenate([p["pair_read"] + np.uint32(nr[k]) for k, p in enumerate(parts)]).astype(np.uint32),
                pair_hap=np.concatenate([p["pair_hap"] + np.uint32(nh[k]) for k, p in enumerate(parts)]).astype(np.uint32))


READ_LENGTHS = (1, 2, 31, 32, 33, 64, 65, 121, 128, 129, 191, 192, 193)


@pytest.mark.parametrize("R", READ_LENGTHS)
def test_every_narrow_class_against_the_oracle(engine, oracle, synth, R):
    """Both ends of every lane-group width (4 lanes to 32 bases, 8 to 64, 16 to 192; 193: the first 64-lane class, which
    keeps the six-operation cell), 121 with row-0 clones on lane 0; haplotypes of 1, 3, 17 and 40-300 bases."""
    parts = [synth.gen_pairhmm_pairs(50, 0xF1FE + 7 * R + k, r_range=(R, R), h_range=hr)
             for k, hr in enumerate(((1, 1), (3, 3), (17, 17), (40, 300)))]
    d = cat(parts)
    assert len(d["pair_read"]) == 200
    _, _, _, _ = check(engine, oracle, d, (0, 50, 100, 150, 199))
    _, _, st = run(engine, d)
    assert st["n_form_deferred_f32"] == (0 if R > 192 else int(np.isin(emulate(d)[2], (STATIC, DYNAMIC)).sum()))


def test_deferral_counts(engine, oracle, synth):
    d = whole_quality_range(synth, 6000)
    want, _ = oracle.batch(d)
    out, used, st = run(engine, d)
    _, _, way = emulate(d)
    n_static, n_dynamic = int((way == STATIC).sum()), int((way == DYNAMIC).sum())
    print(f"static {n_static} dynamic {n_dynamic} device n_form_deferred_f32 {st['n_form_deferred_f32']} n_nhap_f32 {st['n_nhap_f32']}")
    assert n_static > 0 and n_dynamic > 0
    assert st["n_form_deferred_f32"] == n_static + n_dynamic
    assert st["n_nhap_f32"] == int(has_n(d).sum())
    assert_log10_close(out, want)


def test_overflowing_pair_is_deferred(engine, oracle):
    d = overflowing_pair()
    want, wused = oracle.batch(d)
    out, used, st = run(engine, d)
    assert st["n_form_deferred_f32"] == 1 and st["n_nhap_f32"] == 0
    assert used[0] == 0 and wused[0] == 0
    assert_log10_close(out, want)


def test_batch_composition(engine, synth):
    """Some test cases defer (ins / del down to 1: pMM = 0 now and then; neighbouring ins qualities far apart), none has a
    gap-continuation byte of 0, so no wavefront of the second launch takes the plain form: the bits of a test case do not
    depend on its neighbours."""
    n = 6000
    d = synth.gen_pairhmm_pairs(n, 0xC0DE5, r_range=(1, 192), h_range=(1, 300))
    d = with_qualities(d, 5, qual=(6, 60), ins=(1, 127), dele=(1, 127), gcp=(1, 60), zero_ins_del_rate=0.0)
    b = engine.batch(d)
    b.run()
    full = b.results()
    st = b.stats()
    b.close()
    assert 0 < st["n_form_deferred_f32"] < n
    rng = np.random.RandomState(2)
    for _ in range(3):
        idx = np.sort(rng.choice(n, 1500, replace=False))
        sub = dict(d, pair_read=d["pair_read"][idx], pair_hap=d["pair_hap"][idx])
        assert np.array_equal(engine.compute(sub), full[idx])
    way = emulate(d)[2]
    for i in (0, int(np.flatnonzero(way == STATIC)[0]), int(np.flatnonzero(way == 0)[-1])):
        sub = dict(d, pair_read=d["pair_read"][i:i + 1], pair_hap=d["pair_hap"][i:i + 1])
        assert engine.compute(sub)[0].tobytes() == full[i].tobytes(), i


@pytest.fixture
def timed(pkg):
    eng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.TIMING)      # the statistics name the launch that did the most work
    yield eng
    eng.close()


def test_own_launch_against_multi_class_launch(engine, timed, synth):
    """200 test cases of 128 and of 50 bases, three ways.  Alone, the host folds their classes (fewer than 4096 test cases)
    into the widest class of their lane-group width, 16 x 12 and 8 x 8 rows.  Padded with 4100 more of each length they
    run in the 16 x 8 and 8 x 7 kernels, each class in a launch of its own (a multi-class launch needs two classes of
    a lane-width set).  With 4100 reads of 100 and of 20 bases on top, both sets have two classes and share the two
    multi-class launches.  The same bytes all three ways."""
    make = lambda R, k, seed: with_qualities(synth.gen_pairhmm_pairs(k, seed + R, r_range=(R, R), h_range=(40, 300)), R,  # noqa: E731
                                             qual=(6, 60), ins=(1, 127), dele=(1, 127), gcp=(1, 60), zero_ins_del_rate=0.0)
    small = [make(128, 200, 0x5A), make(50, 200, 0x5A)]
    pad = [make(128, 4100, 0x9B), make(50, 4100, 0x9B)]
    more = [make(100, 4100, 0x9B), make(20, 4100, 0x9B)]
    assert np.isin(emulate(cat(small))[2], (STATIC, DYNAMIC)).any()
    alone = engine.compute(cat(small))
    b = timed.batch(cat(small + pad))
    b.run()
    own, st_own = b.results(), b.stats()
    b.close()
    b = timed.batch(cat(small + pad + more))
    b.run()
    multi, st_multi = b.results(), b.stats()
    b.close()
    assert st_own["dominant_kernel"] == "pairhmm_fwd<float, 16, 8>" and st_multi["dominant_kernel"] == "pairhmm_fwd_multi<0>"
    assert alone.tobytes() == own[:400].tobytes()
    assert alone.tobytes() == multi[:400].tobytes()
