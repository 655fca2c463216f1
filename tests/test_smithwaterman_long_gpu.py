"""GPU tests of references of 2049 .. 32 767 bases (MGX_SW_LONG_REF, k_sw_fill_strip) through the C ABI.  Expected CIGAR text,
offset and score come from the oracle (and the reference's own answers from tests/golden/smithwaterman_long.npz); the bar is
identity.  A strip is 2048 reference rows (64 lanes x 32), so the strip seams lie on the multiples of 2048; the multiples of
1024 are tested alike."""
import re

import numpy as np
import pytest

import sw_long as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def long_engine(pkg):
    eng = pkg.SmithWatermanEngine(0, pkg.smithwaterman.LONG_REF)
    yield eng
    eng.close()


def _check(engine, sw_oracle, pairs, strat, params, want=None):
    """one batch against the oracle, pair by pair; -> the engine's stats"""
    w = L.concat(pairs, strat)
    want_c, want_o, want_s = want if want is not None else sw_oracle.batch(w, params)
    got_c, got_o, got_s = engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
    bad = [(len(pairs[q][0]), len(pairs[q][1]), int(strat[q]), got_c[q][:60], want_c[q][:60], int(got_o[q]), int(want_o[q]), int(got_s[q]), int(want_s[q]))
           for q in range(len(pairs)) if got_c[q] != want_c[q] or got_o[q] != want_o[q] or got_s[q] != want_s[q]]
    assert not bad, (params, bad[:4])
    return engine.stats()


SEAM_ROWS = [k * 1024 + d for k in range(2, 7) for d in (-1, 0, 1)] + [2049, 32767]


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("params", L.PARAM_SETS, ids=str)
def test_seams_of_the_strip_size(long_engine, sw_oracle, params, strategy):
    """references one row short of a strip seam, on it and one past it, against alternates around the wavefront's 64 lanes"""
    pairs = [L.make_pair(n, m, 7000 + 7 * n + m) for n in SEAM_ROWS for m in (1, 2, 63, 64, 65, 300)]
    st = _check(long_engine, sw_oracle, pairs, [strategy] * len(pairs), params)
    n_long = sum(len(r) > 2048 for r, _ in pairs)
    assert st["n_pairs_strip"] == n_long == 6 * (len(SEAM_ROWS) - 2)
    assert st["n_strips"] == sum(-(-len(r) // L.STRIP_ROWS) for r, _ in pairs if len(r) > 2048)


def _seam_alternates(ref, S, rng):
    """alternates = reference rows S-150 .. S+150 (1-based) whose alignment has to cross the seam below row S in a given state"""
    row = lambda a, b: ref[a - 1:b]                 # rows a .. b inclusive  # noqa: E731
    other = lambda base: L.ACGT[(int(np.nonzero(L.ACGT == base)[0][0]) + 1) % 4]      # noqa: E731
    mism = row(S - 150, S + 150).copy()
    mism[150] = other(mism[150]); mism[151] = other(mism[151])                         # rows S and S + 1
    return {
        "deletion_across": np.concatenate([row(S - 150, S - 21), row(S + 20, S + 150)]),      # 40 rows, S-20 .. S+19: F extended over the seam
        "deletion_opens_at_S": np.concatenate([row(S - 150, S - 1), row(S + 10, S + 150)]),   # rows S .. S+9
        "deletion_opens_at_S+1": np.concatenate([row(S - 150, S), row(S + 11, S + 150)]),     # rows S+1 .. S+10
        "insertion_at_S": np.concatenate([row(S - 150, S), L.random_bases(rng, 12), row(S + 1, S + 150)]),
        "mismatch_at_S_and_S+1": mism,
    }


@pytest.mark.parametrize("S", [1024, 2048, 3072, 4096])
def test_paths_that_cross_a_seam(long_engine, sw_oracle, S):
    """gaps and mismatches placed on the hand-off: F, H and the diagonal each carry the alignment over a seam"""
    rng = np.random.default_rng(S)
    ref = L.random_bases(rng, max(S + 200, 2300))
    alts = _seam_alternates(ref, S, rng)
    for params in L.PARAM_SETS:
        pairs = [(ref, a) for a in alts.values() for _ in L.STRATEGIES]
        strat = [st for _ in alts for st in L.STRATEGIES]
        w = L.concat(pairs, strat)
        want = sw_oracle.batch(w, params)
        _check(long_engine, sw_oracle, pairs, strat, params, want=want)
        if params == L.STANDARD_NGS:            # the gaps are taken, not clipped: the flanks outweigh them
            by = dict(zip(alts, want[0][::4]))                                         # SOFTCLIP
            assert b"M40D" in by["deletion_across"] and b"M12I" in by["insertion_at_S"], by
            assert b"M10D" in by["deletion_opens_at_S"] and b"M10D" in by["deletion_opens_at_S+1"], by
            assert by["mismatch_at_S_and_S+1"] == b"301M", by


@pytest.mark.parametrize("nrow", [2100, 5000])
def test_boundary_column_beyond_the_first_strip(long_engine, sw_oracle, nrow):
    """INDEL and LEADING_INDEL start rows deep in a later strip at H(i, 0) = open + (i - 1) * extend"""
    ref = L.random_bases(np.random.default_rng(nrow), nrow)
    for params in L.PARAM_SETS:
        _check(long_engine, sw_oracle, [(ref, ref[-50:])] * 2, [10, 11], params)


def test_the_reference_builds_own_outputs(long_engine):
    cases = L.golden_cases()
    want_c, want_o = L.load_golden(cases)
    for params in L.PARAM_SETS:
        idx = [q for q, c in enumerate(cases) if c[2] == params]
        w = L.concat([cases[q][:2] for q in idx], [cases[q][3] for q in idx])
        got_c, got_o = long_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params)
        bad = [(len(cases[q][0]), len(cases[q][1]), cases[q][3]) for x, q in enumerate(idx) if got_c[x] != want_c[q] or got_o[x] != want_o[q]]
        assert not bad, (params, bad[:6])


@pytest.fixture(scope="module")
def mixed_batch(sw_oracle, synth):
    """20 pairs the 16-bit rule admits, 20 for the 32-bit classes, 20 strip pairs, in a seeded permutation; the oracle's answers"""
    short = synth.gen_sw_pairs(20, 501, ref_range=(40, 400), alt_range=(20, 150))
    wide = synth.gen_sw_pairs(20, 502, ref_range=(1800, 2048), alt_range=(500, 700))
    cut = lambda w, p: (w["ref"][int(w["ref_off"][p]):int(w["ref_off"][p + 1])], w["alt"][int(w["alt_off"][p]):int(w["alt_off"][p + 1])])  # noqa: E731
    rng = np.random.default_rng(503)
    rows = [2049, 7000, 4096, 4097] + [int(x) for x in rng.integers(2049, 7001, 16)]
    pool = [(cut(short, p), short["strategy"][p]) for p in range(20)] + [(cut(wide, p), wide["strategy"][p]) for p in range(20)] + \
           [(L.make_pair(n, int(rng.integers(30, 400)), 600 + k), L.STRATEGIES[k % 4]) for k, n in enumerate(rows)]
    order = rng.permutation(len(pool))
    pairs = [pool[q][0] for q in order]; strat = [int(pool[q][1]) for q in order]
    return pairs, strat, sw_oracle.batch(L.concat(pairs, strat), L.STANDARD_NGS)


@pytest.mark.parametrize("paired", ["0", "1"])
def test_mixed_batch(pkg, long_engine, sw_oracle, mixed_batch, monkeypatch, paired):
    """strip pairs among today's classes, in small chunks: the others are treated exactly as a context without the flag treats them"""
    pairs, strat, want = mixed_batch
    monkeypatch.setenv("MGX_SW_PAIRED", paired)
    monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(4 << 20))           # a strip pair takes 4 MiB or more with an alternate of some length
    st = _check(long_engine, sw_oracle, pairs, strat, L.STANDARD_NGS, want=want)
    w = L.concat(pairs, strat)
    got = long_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)
    sub = [q for q in range(len(pairs)) if len(pairs[q][0]) <= 2048]
    assert len(sub) == 40 and st["n_pairs_strip"] == len(pairs) - len(sub) == 20
    plain = pkg.SmithWatermanEngine(0)
    try:
        ws = L.concat([pairs[q] for q in sub], [strat[q] for q in sub])
        sc, so, ss = plain.align_batch(ws["ref_off"], ws["ref"], ws["alt_off"], ws["alt"], ws["strategy"], want_score=True)
        pst = plain.stats()
    finally:
        plain.close()
    assert sc == [got[0][q] for q in sub] and np.array_equal(so, got[1][sub]) and np.array_equal(ss, got[2][sub])
    assert st["n_pairs_i16"] == pst["n_pairs_i16"] and 20 <= pst["n_pairs_i16"] < 40
    assert pst["n_pairs_strip"] == 0 and pst["n_strips"] == 0
    assert st["n_launches"] > 20                                      # chunks of their own


def test_long_element_lists(long_engine, sw_oracle):
    """30 short indels along a 4100-base reference: more than 16 elements, the gather path"""
    rng = np.random.default_rng(66)
    ref = L.random_bases(rng, 4100)
    parts, at = [], 100
    for k in range(30):
        parts.append(ref[at:at + 120])
        if k % 2:
            parts.append(L.random_bases(rng, 3)); at += 120              # insertion
        else:
            at += 123                                                    # deletion of 3
    alt = np.concatenate(parts + [ref[at:at + 120]])
    want = sw_oracle.batch(L.concat([(ref, alt)] * 4, L.STRATEGIES), L.STANDARD_NGS)
    assert all(len(re.findall(rb"\d+[MIDS]", c)) > 16 for c in want[0])
    _check(long_engine, sw_oracle, [(ref, alt)] * 4, L.STRATEGIES, L.STANDARD_NGS, want=want)


def test_long_partner(long_engine, sw_oracle):
    """alternates of thousands of bases under several strips, and the longest reference against a single base"""
    a = L.make_pair(4100, 9000, 71); b = L.make_pair(32767, 1500, 72)
    st = _check(long_engine, sw_oracle, [a, b], [9, 9], L.STANDARD_NGS)
    assert st["n_strips"] == 3 + 16
    for params in L.PARAM_SETS:
        ref = L.random_bases(np.random.default_rng(73), 32767)
        _check(long_engine, sw_oracle, [(ref, ref[20000:20001])] * 4, L.STRATEGIES, params)


def test_align_with_the_flag(long_engine, sw_oracle):
    """mgx_sw_align on a flagged context, with the default capacity and with one that cuts the text (the capacity rule)"""
    ref, alt = L.make_pair(5000, 200, 81)
    for st in L.STRATEGIES:
        for cap in (None, 7):
            want_c, want_o, _ = sw_oracle.align(ref, alt, L.STANDARD_NGS, st, cap=cap)
            got_c, got_o = long_engine.align(ref.tobytes(), alt.tobytes(), L.STANDARD_NGS, st, cigar_length=cap)
            assert got_c == want_c and got_o == want_o, (st, cap)
    assert long_engine.stats()["n_pairs_strip"] == 1 and long_engine.stats()["n_strips"] == 3


def test_limits(pkg, long_engine):
    z = np.full(32768, 65, dtype=np.uint8)
    with pytest.raises(pkg.MgxError, match="32768 bases .limit 32767"):       # reference
        long_engine.align_batch([0, 32768], z, [0, 10], z[:10], [9])
    with pytest.raises(pkg.MgxError, match="32768 bases .limit 32767"):       # alternate
        long_engine.align_batch([0, 10], z[:10], [0, 32768], z, [9])
    with pytest.raises(pkg.MgxError):
        long_engine.align(z.tobytes(), z[:10].tobytes())
    plain = pkg.SmithWatermanEngine(0)
    try:
        with pytest.raises(pkg.MgxError, match="2049 bases .limit 2048"):
            plain.align_batch([0, 2049], z[:2049], [0, 10], z[:10], [9])
    finally:
        plain.close()
