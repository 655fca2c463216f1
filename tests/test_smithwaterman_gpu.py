"""GPU parity tests of the Smith-Waterman path (row F4) through the C ABI, against the oracle and the
golden vectors of the reference's own aligner.  Bar: CIGAR text and offset identical."""
import os

import numpy as np
import pytest

from test_smithwaterman_oracle import cig_bytes, load_gold

pytestmark = pytest.mark.gpu


def test_golden_vectors(sw_engine):
    for k in range(3):
        w, params, cig, off = load_gold(k)
        got_c, got_o = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params)
        assert np.array_equal(got_o, off)
        assert got_c == [cig_bytes(r) for r in cig]


@pytest.mark.parametrize("ref_range,alt_range,n", [((1, 64), (1, 64), 1500), ((60, 130), (20, 150), 800),
                                                   ((250, 520), (100, 300), 300), ((900, 1100), (50, 400), 60),
                                                   ((1500, 2048), (100, 300), 20),
                                                   ((1900, 2048), (4000, 8000), 3)])      # long alternates
def test_random_vs_oracle(sw_engine, sw_oracle, synth, ref_range, alt_range, n):
    """every row class of the fill kernel (1, 2, 4, 8, 16, 32 rows per lane), all strategies"""
    for seed, params in ((11, (25, -50, -110, -6)), (12, (3, -1, -4, -3))):
        w = synth.gen_sw_pairs(n, seed + ref_range[0], ref_range=ref_range, alt_range=alt_range)
        want_c, want_o, want_s = sw_oracle.batch(w, params)
        got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
        assert np.array_equal(got_o, want_o)
        assert np.array_equal(got_s, want_s)
        assert got_c == want_c


@pytest.mark.parametrize("paired", ["0", "1"])
def test_both_shape_families(sw_engine, sw_oracle, synth, monkeypatch, paired):
    """large batches put two pairs on a wavefront (32 lanes each), small ones keep 64 lanes per pair:
    force each family over every row class"""
    monkeypatch.setenv("MGX_SW_PAIRED", paired)
    for k, (rr, n) in enumerate((((1, 70), 300), ((100, 520), 300), ((600, 2048), 24))):
        w = synth.gen_sw_pairs(n, 200 + k, ref_range=rr, alt_range=(5, 260))
        want_c, want_o, _ = sw_oracle.batch(w, (25, -50, -110, -6))
        got_c, got_o = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"])
        assert np.array_equal(got_o, want_o) and got_c == want_c


def test_single_pair_entry_point(sw_engine, sw_oracle):
    """mgx_sw_align == SmithWaterman_align argument for argument, including short text buffers"""
    ref = np.frombuffer(b"ACGTACGTAAACCCGGGTTTACGATCGATCGGCTA", dtype=np.uint8)
    alt = np.frombuffer(b"TTACGTTTACGTAAACGGGTTACGATGATCGGC", dtype=np.uint8)
    for st in (9, 10, 11, 12):
        for cap in (None, 3, 6):
            want_c, want_o, _ = sw_oracle.align(ref, alt, (25, -50, -110, -6), st, cap=cap)
            got_c, got_o = sw_engine.align(ref.tobytes(), alt.tobytes(), (25, -50, -110, -6), st, cigar_length=cap)
            assert got_c == want_c and got_o == want_o


def test_mixed_classes_keep_input_order(sw_engine, sw_oracle, synth):
    """pairs of different row classes interleaved: results come back in input order"""
    parts = [synth.gen_sw_pairs(40, 70 + k, ref_range=r, alt_range=(10, 90)) for k, r in enumerate(((5, 60), (300, 500), (70, 120), (1000, 1300)))]
    order = np.random.default_rng(5).permutation(160)
    refs, alts, strat = [], [], []
    for q in order:
        w = parts[q // 40]; p = q % 40
        refs.append(w["ref"][int(w["ref_off"][p]):int(w["ref_off"][p + 1])]); alts.append(w["alt"][int(w["alt_off"][p]):int(w["alt_off"][p + 1])])
        strat.append(w["strategy"][p])
    ro = np.zeros(161, dtype=np.uint64); ao = np.zeros(161, dtype=np.uint64)
    ro[1:] = np.cumsum([len(r) for r in refs]); ao[1:] = np.cumsum([len(r) for r in alts])
    w = dict(ref_off=ro, ref=np.concatenate(refs), alt_off=ao, alt=np.concatenate(alts), strategy=np.array(strat, dtype=np.uint8))
    want_c, want_o, _ = sw_oracle.batch(w, (25, -50, -110, -6))
    got_c, got_o = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"])
    assert np.array_equal(got_o, want_o) and got_c == want_c


def test_batches_larger_than_the_arena_are_chunked(sw_engine, sw_oracle, synth, monkeypatch):
    """a batch whose back-trace matrices exceed the arena is processed in several chunks"""
    w = synth.gen_sw_pairs(300, 91, ref_range=(40, 300), alt_range=(20, 150))
    want_c, want_o, _ = sw_oracle.batch(w, (25, -50, -110, -6))
    monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(1 << 20))          # about a dozen pairs per chunk
    got_c, got_o = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"])
    assert np.array_equal(got_o, want_o) and got_c == want_c
    assert sw_engine.stats()["n_launches"] >= 8              # one launch per chunk when every pair takes the 16-bit kernel


def test_limits_are_errors_not_faults(pkg, sw_engine):
    z = np.zeros(3000, dtype=np.uint8) + 65
    with pytest.raises(pkg.MgxError):       # reference longer than 2048
        sw_engine.align_batch([0, 2049], z[:2049], [0, 10], z[:10], [9])
    with pytest.raises(pkg.MgxError):       # empty alternate
        sw_engine.align_batch([0, 10], z[:10], [0, 0], z[:0], [9])
    with pytest.raises(pkg.MgxError):       # unknown strategy
        sw_engine.align_batch([0, 10], z[:10], [0, 10], z[:10], [3])
    c, o = sw_engine.align_batch(np.zeros(1, np.uint64), z[:0], np.zeros(1, np.uint64), z[:0], np.zeros(0, np.uint8))
    assert c == [] and len(o) == 0


def _concat(pairs, strategies):
    ro = np.zeros(len(pairs) + 1, dtype=np.uint64); ao = np.zeros(len(pairs) + 1, dtype=np.uint64)
    ro[1:] = np.cumsum([len(r) for r, _ in pairs]); ao[1:] = np.cumsum([len(a) for _, a in pairs])
    return dict(ref_off=ro, ref=np.concatenate([r for r, _ in pairs]), alt_off=ao, alt=np.concatenate([a for _, a in pairs]),
                strategy=np.array(strategies, dtype=np.uint8))


@pytest.mark.parametrize("i16", ["0", "1"])
@pytest.mark.parametrize("paired", ["0", "1"])
def test_packed_16_bit_fill_and_32_bit_fill_agree_with_the_oracle(sw_engine, sw_oracle, synth, monkeypatch, i16, paired):
    """round 3: pairs whose scores provably fit 16 bits are filled two to a lane group with packed arithmetic and
    nibble back-trace (k_sw_fill16); MGX_SW_I16=0 sends every pair through the 32-bit kernel.  Every row class of
    both, odd class sizes (filler jobs), both parameter sets, all strategies."""
    monkeypatch.setenv("MGX_SW_I16", i16)
    monkeypatch.setenv("MGX_SW_PAIRED", paired)
    for k, (rr, ar, n) in enumerate((((1, 40), (1, 60), 501), ((30, 470), (5, 260), 777), ((400, 1100), (20, 200), 101))):
        for params in ((25, -50, -110, -6), (3, -1, -4, -3)):
            w = synth.gen_sw_pairs(n, 900 + k, ref_range=rr, alt_range=ar)
            want_c, want_o, want_s = sw_oracle.batch(w, params)
            got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
            assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c
            st = sw_engine.stats()
            assert (st["n_pairs_i16"] > 0) == (i16 == "1")


def test_16_bit_admission(sw_engine, sw_oracle, synth):
    """the 16-bit kernel takes a pair only when the bound on its scores holds: large parameters, long references and
    long alternates fall back pair by pair, inside one batch"""
    w = synth.gen_sw_pairs(200, 77, ref_range=(50, 300), alt_range=(20, 150))
    for params, expect in (((25, -50, -110, -6), 200), ((2500, -5000, -11000, -600), 0), ((25, -50, 110, 6), None)):
        want_c, want_o, want_s = sw_oracle.batch(w, params)
        got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
        assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c
        if expect is not None:
            assert sw_engine.stats()["n_pairs_i16"] == expect
    parts = [synth.gen_sw_pairs(40, 300 + k, ref_range=r, alt_range=a) for k, (r, a) in enumerate((((100, 400), (50, 150)), ((1800, 2048), (500, 700)),
                                                                                                   ((200, 300), (3000, 5000))))]
    pairs, strat = [], []
    for q in np.random.default_rng(9).permutation(120):
        v = parts[q // 40]; p = q % 40
        pairs.append((v["ref"][int(v["ref_off"][p]):int(v["ref_off"][p + 1])], v["alt"][int(v["alt_off"][p]):int(v["alt_off"][p + 1])]))
        strat.append(v["strategy"][p])
    w = _concat(pairs, strat)
    want_c, want_o, want_s = sw_oracle.batch(w, (25, -50, -110, -6))
    got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
    assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c
    assert 40 <= sw_engine.stats()["n_pairs_i16"] < 120      # the first group whole; long references with long alternates and 3000-base alternates not


def test_16_bit_fill_at_the_ends_of_its_range(sw_engine, sw_oracle):
    """sequences that drive the scores to the bounds the admission rule computes: nothing but mismatches (lowest H),
    nothing but matches (highest), one long gap, at the largest lengths the rule admits for these parameters"""
    A, Cc = np.full(1000, 65, np.uint8), np.full(1000, 67, np.uint8)
    rng = np.random.default_rng(3)
    rnd = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1000)]
    pairs, strat = [], []
    for st in (9, 10, 11, 12):
        for ref, alt in ((A[:1000], Cc[:300]), (A[:1000], A[:300]), (rnd[:1000], rnd[350:650]), (rnd[:1000], np.concatenate([rnd[:150], rnd[850:1000]])),
                         (A[:300], Cc[:300]), (rnd[:300], rnd[:300]), (Cc[:7], A[:300]), (A[:1000], Cc[:1])):
            pairs.append((ref, alt)); strat.append(st)
    w = _concat(pairs, strat)
    for params in ((25, -50, -110, -6), (3, -1, -4, -3), (100, -100, -30, -30)):
        want_c, want_o, want_s = sw_oracle.batch(w, params)
        got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_o, want_o) and got_c == want_c
        assert sw_engine.stats()["n_pairs_i16"] > 0


def test_32bit_fill_paired_and_unpaired(sw_engine, sw_oracle, synth, monkeypatch):
    """the 32-bit kernel for every pair (MGX_SW_I16=0), with two pairs per wavefront and with one, on references both
    longer and shorter than their alternates"""
    monkeypatch.setenv("MGX_SW_I16", "0")
    for paired in ("0", "1"):
        monkeypatch.setenv("MGX_SW_PAIRED", paired)
        w = synth.gen_sw_pairs(400, 55, ref_range=(30, 600), alt_range=(5, 300))
        want_c, want_o, want_s = sw_oracle.batch(w, (25, -50, -110, -6))
        got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
        assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c


def test_largest_sizes_and_many_chunks(sw_engine, sw_oracle, synth, monkeypatch):
    """the largest lengths the ABI takes (reference 2048, alternate 32 767: the 32-bit kernel, one pair per chunk-sized
    arena) and a batch of pairs at the 16-bit kernel's admission edge cut into many chunks by a small arena"""
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.integers(0, 4, 2048)]
    alt_long = np.concatenate([acgt[rng.integers(0, 4, 15000)], ref[100:1900], acgt[rng.integers(0, 4, 32767 - 15000 - 1800)]])
    w = _concat([(ref, alt_long), (ref[:2047], alt_long[:30000]), (ref, ref[5:2040])], [9, 12, 10])
    want_c, want_o, want_s = sw_oracle.batch(w, (25, -50, -110, -6))
    got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
    assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c
    assert sw_engine.stats()["n_pairs_i16"] == 0
    monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(16 << 20))
    w = synth.gen_sw_pairs(600, 4242, ref_range=(700, 1000), alt_range=(100, 300))
    want_c, want_o, want_s = sw_oracle.batch(w, (25, -50, -110, -6))
    got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
    assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c
    st = sw_engine.stats()
    assert st["n_pairs_i16"] == 600 and st["n_launches"] >= 4


def test_stats_of_the_fixed_batch(pkg, sw_oracle, monkeypatch):
    """sw_frontier.FIXED_LENS under both lane-group families and both fills: what the library launches and reserves is what
    tests/test_sw_layout_host.py holds csrc/sw_layout.h to on the CPU (the same literal numbers), and the answers are the oracle's"""
    import sw_frontier as F
    import sw_long as L
    pairs = [L.make_pair(n, m, 9000 + q) for q, (n, m) in enumerate(F.FIXED_LENS)]
    w = L.concat(pairs, F.FIXED_STRATEGIES)
    want_c, want_o, want_s = sw_oracle.batch(w, F.STANDARD_NGS)
    eng = pkg.SmithWatermanEngine(0, pkg.smithwaterman.LONG_REF)              # the batch holds references of 2049 and 4097 bases
    try:
        for (paired, i16), want in sorted(F.FIXED_STATS.items()):
            monkeypatch.setenv("MGX_SW_PAIRED", str(paired))
            monkeypatch.setenv("MGX_SW_I16", str(i16))
            got_c, got_o, got_s = eng.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], F.STANDARD_NGS, want_score=True)
            assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s) and got_c == want_c, (paired, i16)
            st = eng.stats()
            assert tuple(int(st[k]) for k in F.FIXED_STAT_KEYS) == want, (paired, i16)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# The packed 16-bit fill along its admission frontier.  Whether a pair is admitted is asked of the host driver
# (tests/cpp/sw_i16_rule_driver.cpp over csrc/sw_i16_rule.h), never of the device; CIGAR, offset and score come from the
# oracle; n_pairs_i16 must equal the driver's count, so a pair meant for the 16-bit kernel cannot pass through the 32-bit one.
import sw_frontier as F  # noqa: E402


@pytest.fixture(scope="module")
def rule_driver(tmp_path_factory):
    return F.Driver(tmp_path_factory.mktemp("sw_i16_rule"), sanitize=False)


def _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, families, monkeypatch, want=None):
    """one batch through the engine under each lane-group family; -> the driver's admission per pair"""
    lens = [(len(r), len(a)) for r, a in pairs]
    adm = rule_driver.admitted(params, lens)
    w = F.concat(pairs, strat)
    want_c, want_o, want_s = sw_oracle.batch(w, params)
    for paired in families:
        monkeypatch.setenv("MGX_SW_PAIRED", paired)
        if want is not None:             # the partners the batch was built for do meet
            assert set(F.lane_groups(lens, adm, paired == "1")) == set(want(paired == "1")), (params, paired)
        got_c, got_o, got_s = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
        bad = [q for q in range(len(pairs)) if got_s[q] != want_s[q] or got_o[q] != want_o[q] or got_c[q] != want_c[q]]
        assert not bad, (params, paired, [(lens[q], int(strat[q]), adm[q]) for q in bad[:8]])
        assert sw_engine.stats()["n_pairs_i16"] == sum(adm), (params, paired)
    return adm


@pytest.mark.parametrize("paired", ["0", "1"])
@pytest.mark.parametrize("params", F.REAL_SETS, ids=str)
def test_frontier_of_the_real_parameters_in_every_row_class(sw_engine, sw_oracle, rule_driver, monkeypatch, params, paired):
    """for a reference at the top or the bottom of every row class of the family: the largest admitted alternate (bisection
    over the driver), one base less, and one more -- which comes back through the 32-bit kernel, as the count shows.
    Extremal sequences and strategies rotate over the classes."""
    pairs, strat, expect = [], [], []
    for c, (r, n_lo, n_hi) in enumerate(F.class_lengths(paired == "1")):
        n = n_hi if c % 2 == 0 else n_lo
        m = rule_driver.largest_admitted_alt(params, n)
        for d, mm in enumerate((m - 1, m, m + 1)):
            if mm < 1:
                continue
            for e in range(2):
                pairs.append(F.extremal(F.EXTREMAL_KINDS[(3 * c + 2 * d + e) % 8], n, mm)); strat.append(F.STRATEGIES[(c + d + e) % 4])
                expect.append(mm <= m)
    adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, (paired,), monkeypatch)
    assert adm == expect and any(adm) and not all(adm)


@pytest.mark.parametrize("name,params,side", F.SCALED_SETS, ids=[s[0] for s in F.SCALED_SETS])
def test_frontier_of_scaled_parameters_cuts_through_the_batch(sw_engine, sw_oracle, rule_driver, monkeypatch, name, params, side):
    """the dense boxes of test_sw_i16_rule_host.py as one batch per parameter set, in row-major order of (n, m): admitted and
    refused pairs interleave.  One rotating extremal pair per point, all of them under every strategy within two steps of
    the frontier."""
    pts = [(n, m) for n in range(1, side + 1) for m in range(1, side + 1)]
    ok = dict(zip(pts, rule_driver.admitted(params, pts)))
    pairs, strat = [], []
    for q, (n, m) in enumerate(pts):
        hood = [ok.get((n + d, m + e), False) for d in range(-2, 3) for e in range(-2, 3) if n + d >= 1 and m + e >= 1]
        if any(hood) and not all(hood):
            for st in F.STRATEGIES:
                for kind in F.EXTREMAL_KINDS:
                    pairs.append(F.extremal(kind, n, m)); strat.append(st)
        else:
            pairs.append(F.extremal(F.EXTREMAL_KINDS[q % 8], n, m)); strat.append(F.STRATEGIES[(q // 8) % 4])
    adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, ("0", "1"), monkeypatch)
    assert 0 < sum(adm) < len(adm)
    flips = sum(1 for a, b in zip(adm, adm[1:]) if a != b)
    assert flips >= side // 2                # the frontier runs through the batch, not along its end


@pytest.mark.parametrize("params", [F.STANDARD_NGS, F.FLAT], ids=str)
def test_frontier_pair_with_an_unequal_partner(sw_engine, sw_oracle, rule_driver, monkeypatch, params):
    """A frontier pair (reference at the top of its row class, largest admitted alternate) sharing its lane group with a very
    different partner.  The admitted pairs of a batch are launched class by class and, inside a class, longest alternate
    first, equal alternates in input order; neighbours of that order share a lane group, the first in the low halves (kJobHalf
    clear), the second in the high halves (kJobHalf set).  So every class below holds exactly the two pairs that are to meet
    (sw_frontier.lane_groups restates the order and the test checks the meeting):
      (a) class of 1 row per lane: the frontier pair and a 1 x 1 pair -> frontier low, 1 x 1 high
      (b) two classes: the frontier pair and a pair of the same class with a quarter of the alternate -> frontier low
      (c) two classes: the frontier pair alone -> frontier low, a filler job high (odd class size)
      (d) three classes: the frontier pair and, listed before it, the frontier pair of the shortest reference of the class,
          whose alternate is at least as long -> frontier HIGH, under a partner that sweeps on after its last column
    A shorter partner cannot sit in the low halves and a filler cannot either: the order puts the longer alternate first."""
    fam = {}
    for paired in (False, True):
        cl = {r: (lo, hi) for r, lo, hi in F.class_lengths(paired)}
        big = {r: rule_driver.largest_admitted_alt(params, cl[r][1]) for r in cl}
        usable = [r for r in cl if r > 1 and big[r] >= 8]              # long references admit no alternate under large parameters
        assert big[1] >= 8 and len(usable) >= 7
        picks = [usable[(len(usable) - 1) * x // 6] for x in range(7)]              # spread from 2 rows per lane to the most
        roles = dict(b=(picks[1], picks[5]), c=(picks[2], picks[4]), d=(picks[0], picks[3], picks[6]))
        big_lo = {r: rule_driver.largest_admitted_alt(params, cl[r][0]) for r in roles["d"]}
        assert len(set(picks)) == 7 and all(big_lo[r] >= big[r] for r in big_lo)
        fam[paired] = (cl, big, big_lo, roles)
    for k, kind in enumerate(F.EXTREMAL_KINDS):
        for paired in (False, True):
            cl, big, big_lo, roles = fam[paired]
            st = F.STRATEGIES[k % 4]
            rnd = F.extremal("gap_middle", 1, 1)
            pairs, strat, groups = [rnd, F.extremal(kind, cl[1][1], big[1])], [F.STRATEGIES[(k + 1) % 4], st], [(1, 0)]          # (a)
            for r in roles["b"]:                                                                                           # (b)
                q = len(pairs)
                pairs += [F.extremal("gap_last", cl[r][1] - 3, big[r] // 4), F.extremal(kind, cl[r][1], big[r])]
                strat += [F.STRATEGIES[(k + 2) % 4], st]; groups.append((q + 1, q))
            for r in roles["c"]:                                                                                           # (c)
                pairs.append(F.extremal(kind, cl[r][1], big[r])); strat.append(st); groups.append((len(pairs) - 1, None))
            for r in roles["d"]:                                                                                       # (d)
                q = len(pairs)
                pairs += [F.extremal(F.EXTREMAL_KINDS[(k + 3) % 8], cl[r][0], big_lo[r]), F.extremal(kind, cl[r][1], big[r])]
                strat += [F.STRATEGIES[(k + 3) % 4], st]; groups.append((q, q + 1))
            adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, ("1" if paired else "0",), monkeypatch,
                                  want=lambda p, g=groups: g)
            assert all(adm)


def test_frontier_at_the_lds_limit_of_the_alternate(sw_engine, sw_oracle, rule_driver, monkeypatch):
    """alternates of 4095 and 4096 bases (two of them fill the LDS stage of a lane group) are admitted, 4097 are not, under
    parameters whose scores allow all three; two 4096-base alternates in one lane group; one with a short partner"""
    params = F.ORIGINAL_DEFAULT
    pairs, strat, expect = [], [], []
    for a, n in enumerate((1, 200, 2048)):
        for b, m in enumerate((4095, 4096, 4097)):
            for e in range(2):
                pairs.append(F.extremal(F.EXTREMAL_KINDS[(3 * a + 2 * b + 5 * e) % 8], n, m)); strat.append(F.STRATEGIES[(a + b + e) % 4])
                expect.append(m <= 4096)
    adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, ("0", "1"), monkeypatch)
    assert adm == expect
    # references of 199 / 200 bases share a row class in both families, and so do 290 / 300; each class holds one lane group
    pairs = [F.extremal("gap_middle", 200, 4096), F.extremal("all_mismatch", 199, 4096), F.extremal("gap_first", 290, 5), F.extremal("all_match", 300, 4096)]
    adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, [10, 9, 12, 11], ("0", "1"), monkeypatch,
                          want=lambda p: [(0, 1), (3, 2)])
    assert all(adm)


def test_frontier_pairs_in_many_chunks(sw_engine, sw_oracle, rule_driver, monkeypatch):
    """largest-admitted pairs under a small arena: the chunk bound holds for the 16-bit layout at its largest"""
    params = F.STANDARD_NGS
    pairs, strat = [], []
    for q in range(40):
        n = (1000, 2048, 640, 64)[q % 4]
        pairs.append(F.extremal(F.EXTREMAL_KINDS[q % 8], n, rule_driver.largest_admitted_alt(params, n))); strat.append(F.STRATEGIES[(q // 8) % 4])
    monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(4 << 20))
    adm = _frontier_batch(sw_engine, sw_oracle, rule_driver, params, pairs, strat, ("0",), monkeypatch)
    assert all(adm) and sw_engine.stats()["n_launches"] >= 5
