"""The pairs of tests/sw_trace_cases.py -- one family per seam of the back-trace kernel: the register path of the end cell, match runs
around the 64-cell diagonal cache, gaps on its boundaries, end-cell ties, element lists around the compact copy, degenerate shapes,
strips -- through the C ABI under both fills and both lane-group families.  Text, offset and score are the oracle's; the bar is identity.
tests/test_sw_trace_host.py shows on the CPU that the families reach their seams."""
import numpy as np
import pytest

import sw_long as L
import sw_trace_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


@pytest.fixture(scope="module")
def want(sw_oracle, cases):
    return C.expected(sw_oracle, cases)


@pytest.fixture(scope="module")
def long_engine(pkg):
    eng = pkg.SmithWatermanEngine(0, pkg.smithwaterman.LONG_REF)
    yield eng
    eng.close()


@pytest.mark.parametrize("i16", ["0", "1"])
@pytest.mark.parametrize("paired", ["0", "1"])
def test_all_families_in_one_batch(sw_engine, long_engine, cases, want, monkeypatch, paired, i16):
    monkeypatch.setenv("MGX_SW_PAIRED", paired)
    monkeypatch.setenv("MGX_SW_I16", i16)
    seen = 0
    for long in (False, True):
        for params in (C.STANDARD_NGS, C.ORIGINAL_DEFAULT):
            idx = [q for q, c in enumerate(cases) if c["params"] == params and (len(c["ref"]) > 2048) == long]
            if not idx:
                continue
            w = L.concat([(cases[q]["ref"], cases[q]["alt"]) for q in idx], [cases[q]["strategy"] for q in idx])
            eng = long_engine if long else sw_engine
            got_c, got_o, got_s = eng.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params, want_score=True)
            bad = [(cases[q]["name"], got_c[x], int(got_o[x]), int(got_s[x]), want[q][:3]) for x, q in enumerate(idx)
                   if (got_c[x], got_o[x], got_s[x]) != want[q][:3]]
            assert not bad, (params, len(bad), bad[:4])
            st = eng.stats()
            assert (st["n_pairs_i16"] > 0) == (i16 == "1" and not long) and st["n_pairs_strip"] == (len(idx) if long else 0)
            seen += len(idx)
    assert seen == len(cases)


def test_short_text_buffers(sw_engine, cases, want):
    """the element lists around the compact copy through mgx_sw_align, whose caller names the text's capacity"""
    capped = [(c, w) for c, w in zip(cases, want) if c["caps"]]
    assert len(capped) == 16
    for c, (text, offset, _, cap_texts) in capped:
        for cap, cap_text in [(None, text)] + sorted(cap_texts.items()):
            got_c, got_o = sw_engine.align(c["ref"].tobytes(), c["alt"].tobytes(), c["params"], c["strategy"], cigar_length=cap)
            assert got_c == cap_text and got_o == offset, (c["name"], cap)
