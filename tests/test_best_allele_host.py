"""The best-haplotype rule of the realignment call (csrc/best_allele_rule.h) on the CPU: tests/cpp/best_allele_driver.cpp, built with
-Werror under AddressSanitizer + UBSan and with -ffp-contract=off like the library, folds the header's two merges serially, in 64
strided lanes joined by a butterfly (the kernel's grouping) and in random split trees; every grouping must give what the sequential
restatement of AlleleLikelihoods::searchBestAllele gives (realign_cases.search_best_allele).  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import realign_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-genomic-data-processing_amd", "csrc")
GROUPINGS = ("serial", "64 lanes + butterfly", "tree", "tree", "tree")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    work = tmp_path_factory.mktemp("best_allele")
    exe = os.path.join(str(work), "best_allele_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "best_allele_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")

    def run(rows):
        path = os.path.join(str(work), "rows.txt")
        with open(path, "w") as f:
            for _, v, p in rows:
                nums = list(v) + ([] if p is None else list(p))
                f.write("%d %d %s\n" % (p is not None, len(v), " ".join(float(x).hex() for x in nums)))
        res = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
        assert res.returncode == 0 and not res.stderr, res.stdout[-1000:] + res.stderr[-4000:]
        got = [[int(x) for x in line.split()] for line in res.stdout.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def test_the_restatement_on_hand_made_rows():
    """what the rule must do, stated by hand: the restatement itself is the yardstick of everything else"""
    S = RC.search_best_allele
    assert S([-1.0], [5.0]) == 0 and S([RC.NEG_INF] * 3, [1.0, 2.0, 3.0]) == 0
    assert S([-2.0, -1.0, -1.0], None) == 1                                   # the first of the maxima
    assert S([-1.0, -1.1, -3.0], [0.0, 1.0, 9.0]) == 1                        # inside the threshold: priority decides, 2 is no candidate
    assert S([-1.0, -1.1, -3.0], [1.0, 1.0, 9.0]) == 0                        # strict: an equal priority keeps the likelihood-best
    assert S([-1.0, -1.1, -1.05], [0.0, 3.0, 3.0]) == 1                       # the first of two candidates with the maximum priority
    assert S([-1.0, -1.5], [0.0, 1.0]) == 0                                   # beyond the threshold: not entered


def test_every_grouping_equals_the_sequential_restatement(driver):
    rows = RC.rule_rows()
    got = driver(rows)
    changed = 0
    for (name, v, p), g in zip(rows, got):
        want = RC.search_best_allele(v, p)
        assert g == [want] * len(GROUPINGS), (name, dict(zip(GROUPINGS, g)), want, list(v), None if p is None else list(p))
        changed += p is not None and want != RC.search_best_allele(v, None)
    assert {len(v) for _, v, _ in rows} >= set(RC.WIDTHS) and any(p is None for _, _, p in rows)
    assert changed > 50, changed                                              # the tie-break decides often enough to be tested
    # the threshold's two sides are both taken: a gap of exactly 0.2 in log10 and its neighbours do not all fall on one side
    sides = {(v.max() * RC.LN10 - x * RC.LN10 < RC.THRESHOLD, v.max() * RC.LN10 - x * RC.LN10 > RC.THRESHOLD)
             for _, v, _ in rows if np.isfinite(v.max()) for x in v if abs((v.max() - x) - 0.2) < 1e-12}
    assert len(sides) >= 2, sides
