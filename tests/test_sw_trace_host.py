"""The Smith-Waterman back-trace rules (csrc/sw_trace_rule.h) on the CPU: tests/cpp/sw_trace_driver.cpp, built with -Werror under
AddressSanitizer + UBSan, fills every pair of tests/sw_trace_cases.py with the kernels' 32-bit cell, stores the result through the
header's addresses in every form the pair admits (32-bit with 64 and 32 lanes, strips, 16-bit nibbles as the low and the high half), and
runs the end-cell fold and the walk serially, over 64 emulated lanes, and with the end cell replayed from 64-candidate masks.  Every
form and every way must give the oracle's text, offset and score, and the text under a short capacity.  The counters of the 64-lane
run show that each family reaches the seam it was built for.  No GPU, nothing loaded into Python but the oracle."""
import os
import subprocess

import pytest

import sw_frontier as F
import sw_trace_cases as C

FORMS32 = ("b32g64", "b32g32")
FORMS16 = ("i16g64lo", "i16g64hi", "i16g32lo", "i16g32hi")
WAYS = ("serial", "lanes", "replay")


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


@pytest.fixture(scope="module")
def driven(cases, tmp_path_factory):
    """the driver's output for all cases, one process: per case {form: {way: (score, mi, mj, offset, n_elems, text, cap texts)} or None}
    and {form: (refetches, longest run, candidates)}"""
    work = str(tmp_path_factory.mktemp("sw_trace"))
    exe = os.path.join(work, "sw_trace_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-I", F.CSRC, os.path.join(F.ROOT, "tests", "cpp", "sw_trace_driver.cpp"), "-o", exe])
    path = os.path.join(work, "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            f.write("%d %d %d %d %d %s %s %s\n" % (*c["params"], c["strategy"], ",".join(map(str, c["caps"])) or "-",
                                                  c["ref"].tobytes().decode(), c["alt"].tobytes().decode()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=1800)
    assert res.returncode == 0 and not res.stderr, res.stdout[-1000:] + res.stderr[-4000:]
    results = [dict() for _ in cases]
    counters = [dict() for _ in cases]
    for line in res.stdout.splitlines():
        kind, q, form, *v = line.split()
        q = int(q)
        if kind == "skip":
            results[q][form] = None
        elif kind == "cnt":
            counters[q][form] = tuple(int(x) for x in v)
        else:
            way, score, mi, mj, offset, n_elems, text, caps = v
            text = b"" if text == "-" else text.encode()
            caps = [] if caps == "-" and not cases[q]["caps"] else [b"" if t == "-" else t.encode() for t in caps.split(",")]
            results[q].setdefault(form, {})[way] = (int(score), int(mi), int(mj), int(offset), int(n_elems), text, caps)
    return results, counters


@pytest.fixture(scope="module")
def want(sw_oracle, cases):
    return C.expected(sw_oracle, cases)


def test_every_form_and_way_equals_the_oracle(cases, driven, want):
    results, _ = driven
    bad = []
    for c, forms, (text, offset, score, cap_texts) in zip(cases, results, want):
        assert set(forms) == set(FORMS32 + FORMS16 + ("strip",)), c["name"]
        assert (forms["strip"] is not None) == (len(c["ref"]) > 2048) == (forms["b32g64"] is None) == (forms["b32g32"] is None), c["name"]
        for form, ways in forms.items():
            if ways is None:
                continue
            assert set(ways) == set(WAYS), (c["name"], form)
            for way, got in ways.items():
                if (got[5], got[3], got[0], got[6]) != (text, offset, score, [cap_texts[k] for k in c["caps"]]) or got[:5] != ways["serial"][:5]:
                    bad.append((c["name"], form, way, got, (text, offset, score)))
    assert not bad, (len(bad), bad[:5])


def test_every_form_is_exercised_in_every_family_it_applies_to(cases, driven):
    """the strip form applies to the long references alone and is their only 32-bit form; the 16-bit form needs the admission rule's
    consent (sw_i16_rule.h), which every family of short pairs has for some pair under the standard parameters"""
    results, _ = driven
    seen = {fam: set() for fam in C.FAMILIES}
    for c, forms in zip(cases, results):
        seen[c["family"]] |= {form for form, ways in forms.items() if ways is not None}
    assert set(seen) == {c["family"] for c in cases}
    for fam, forms in seen.items():
        assert forms == ({"strip"} if fam == "long_ref" else set(FORMS32 + FORMS16)), (fam, forms)


def test_each_family_reaches_its_seam(cases, driven, want):
    results, counters = driven
    for c, forms, cnt, (text, _, _, _) in zip(cases, results, counters, want):
        w = c["want"]
        for form, (refetches, longest, candidates) in cnt.items():
            assert "run" not in w or longest == w["run"], (c["name"], form, longest)
            assert refetches >= w.get("refetches", 1), (c["name"], form, refetches)
            assert candidates >= w.get("candidates", 1), (c["name"], form, candidates)
            assert "n_elems" not in w or forms[form]["lanes"][4] == w["n_elems"], (c["name"], form)
        assert "text" not in w or text == w["text"].encode(), (c["name"], text)
    by = lambda fam: [c for c in cases if c["family"] == fam]          # noqa: E731
    assert {len(c["ref"]) + len(c["alt"]) for c in by("register_seam")} >= {C.EDGE_CELLS - 1, C.EDGE_CELLS, C.EDGE_CELLS + 1}
    assert {c["want"]["n_elems"] for c in by("elements") if c["want"]} >= {C.COMPACT_ELEMS - 1, C.COMPACT_ELEMS, C.COMPACT_ELEMS + 1, 40}
    assert all(c["caps"] == (3, 6) for c in by("elements"))
    assert len(by("random")) >= 300 and {c["strategy"] for c in by("random")} == set(C.STRATEGIES)
    assert {c["params"] for c in by("random")} == {C.STANDARD_NGS, C.ORIGINAL_DEFAULT}
