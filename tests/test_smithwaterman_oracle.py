"""CPU tests of the Smith-Waterman oracle (oracle/smithwaterman_oracle.c): against the golden vectors
produced by the reference's own aligner and against that aligner's answers on further inputs (live when oracle/_ref is
present, else as stored in tests/golden/reference_answers.npz)."""
import os

import numpy as np

from conftest import ROOT, reference_answers

GOLD = os.path.join(ROOT, "tests", "golden", "smithwaterman.npz")
SW_KEYS = ("ref_off", "ref", "alt_off", "alt", "strategy")


def load_gold(k):
    g = np.load(GOLD)
    w = {key: g[f"p{k}_{key}"] for key in ("ref_off", "ref", "alt_off", "alt", "strategy")}
    return w, tuple(int(x) for x in g[f"p{k}_params"]), g[f"p{k}_cigar"], g[f"p{k}_offset"]


def cig_bytes(row):
    z = np.nonzero(row == 0)[0]
    return bytes(row[:z[0]]) if len(z) else bytes(row)


def test_oracle_matches_golden_vectors(sw_oracle):
    for k in range(3):
        w, params, cig, off = load_gold(k)
        got_c, got_o, _ = sw_oracle.batch(w, params)
        assert np.array_equal(got_o, off)
        assert got_c == [cig_bytes(r) for r in cig]


def test_oracle_matches_reference_build(sw_oracle, sw_ref, synth):
    for seed, params in ((1, (25, -50, -110, -6)), (2, (3, -1, -4, -3)), (3, (1, -2, -3, -1))):
        w = synth.gen_sw_pairs(300, seed, ref_range=(1, 150), alt_range=(1, 120))
        stride = 2 * 150 + 40
        cig, off = reference_answers(f"sw_live_{seed}", [w[k] for k in SW_KEYS] + [np.array(params)],
                                     sw_ref and (lambda: sw_ref.batch(w, params, stride)))
        got_c, got_o, _ = sw_oracle.batch(w, params)
        assert np.array_equal(got_o, off)
        assert got_c == [cig_bytes(r) for r in cig]


def test_text_capacity_rule(sw_oracle, sw_ref):
    """An element whose text does not fit the buffer is skipped (PairWiseSW.h:431-436)."""
    ref = np.frombuffer(b"ACGTACGTAAACCCGGGTTT", dtype=np.uint8); alt = np.frombuffer(b"ACGTTTACGTAAACGGGTT", dtype=np.uint8)
    cases = [(cap, st) for cap in (2, 3, 5, 8, 40) for st in (9, 10, 11, 12)]

    def live():
        res = [sw_ref.align(ref, alt, (3, -1, -4, -3), st, cap=cap) for cap, st in cases]
        return np.array([c.ljust(40, b"\0") for c, _ in res]), np.array([o for _, o in res], dtype=np.int32)
    rcs, ros = reference_answers("sw_text_capacity", [ref, alt, np.array(cases)], sw_ref and live)
    for (cap, st), rc, ro in zip(cases, rcs, ros):
        c, o, _ = sw_oracle.align(ref, alt, (3, -1, -4, -3), st, cap=cap)
        assert c == rc and o == ro
