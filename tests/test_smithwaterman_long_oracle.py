"""CPU test of the Smith-Waterman oracle on references of more than 2048 bases (the range MGX_SW_LONG_REF opens) against the
reference's own aligner: live where oracle/_ref is built, and against its stored answers (tests/golden/smithwaterman_long.npz,
written by tests/golden/make_golden_smithwaterman_long.py) everywhere."""
import numpy as np

import sw_long


def test_oracle_matches_the_reference_build_on_long_references(sw_oracle, sw_ref):
    cases = sw_long.golden_cases()
    assert len(cases) == 8 * (len(sw_long.SHAPES) + len(sw_long.SEAM_SHAPES))
    assert max(len(r) for r, _, _, _ in cases) == 32767 and min(len(a) for _, a, _, _ in cases) == 1
    want_c, want_o = sw_long.load_golden(cases)
    bad = []
    for q, (ref, alt, params, st) in enumerate(cases):
        c, o, _ = sw_oracle.align(ref, alt, params, st)
        if c != want_c[q] or o != want_o[q]:
            bad.append((len(ref), len(alt), params, st, c, want_c[q], o, int(want_o[q])))
        if sw_ref is not None:          # the build's answers today are the stored ones
            rc, ro = sw_ref.align(ref, alt, params, st)
            assert rc == want_c[q] and ro == want_o[q], (len(ref), len(alt), params, st)
    assert not bad, bad[:4]
    assert any(b"D" in c for c in want_c) and len(set(np.asarray(want_o).tolist())) > 10      # the answers are not trivial ones
