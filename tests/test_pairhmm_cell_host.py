"""The PairHMM cell forms of csrc/pairhmm_cell.h on the host, through tools/cell_emulator.cpp:
  * every fp32 `res` bit of forms 1, 3 and 4, and the way every test case goes under form 4, equal tests/golden/pairhmm_cell_bits.npz,
    which tests/golden/make_golden_pairhmm_cell.py wrote before the forms moved into the header -- a change to the header that is meant to
    leave the numerics alone has to leave these alone.  The tables' bits are compared first: another libm is not a changed cell;
  * tests/cpp/pairhmm_cell_driver.cpp, built with -Werror under AddressSanitizer + UBSan at -O1, prints the bits the -O2 shared library
    returns for the edge pairs: the header's rounding does not depend on the optimisation level, and the sweep stays inside its arrays.
No GPU; nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pairhmm_fiveop_cases import (CSRC, DYNAMIC, FIVE, HAP_N, LONG, SRC, STATIC, TABLES, cell_bits_cases, emulate_res, emulator_tables,
                                  one_pair)

FORMS = (1, 3, 4)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pairhmm_cell_bits.npz"))


@pytest.fixture(scope="module")
def cases(synth):
    return cell_bits_cases(synth)


def test_tables_have_the_goldens_bits(golden):
    got = emulator_tables()
    for name in TABLES:
        differ = int((got[name].view(np.uint32) != golden["table_" + name]).sum())
        assert differ == 0, f"table {name}: {differ} entries differ from the golden's: this machine's libm builds other tables, the cells are not at fault"


def test_every_bit_and_every_way_equals_the_golden(golden, cases):
    test_tables_have_the_goldens_bits(golden)
    ways, form0 = [], 0
    for name, d in cases:
        for form in FORMS:
            res, way = emulate_res(d, form)
            bad = np.flatnonzero(res.view(np.uint32) != golden[f"{name}_res{form}"])
            assert bad.size == 0, f"{name}, form {form}: {bad.size} results differ, first at test case {bad[0]}"
        assert np.array_equal(way, golden[f"{name}_way"]), name
        ways.append(way)
        ro = d["read_off"].astype(np.int64)
        zero = np.concatenate([[0], np.cumsum((d["gcp"] & 127) == 0)])
        form0 += int(((zero[ro[1:]] - zero[ro[:-1]])[d["pair_read"]] > 0).sum())
    count = np.bincount(np.concatenate(ways), minlength=5)
    print("ways", count.tolist(), "form 0", form0)
    assert min(count[w] for w in (FIVE, STATIC, DYNAMIC, HAP_N, LONG)) > 0 and form0 > 0


def test_sanitized_driver_prints_the_librarys_bits(tmp_path, cases):
    edge = [d for name, d in cases if name in ("overflow", "r1_h1", "r192", "r193")]
    edge.append(one_pair(b"", 0, 0, 0, 0, b"ACGT"))                     # a read of 0 bases: the boundary row alone
    exe, batch = str(tmp_path / "pairhmm_cell_san"), str(tmp_path / "batch.txt")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-ffp-contract=off", "-fopenmp", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pairhmm_cell_driver.cpp")] + SRC + ["-o", exe])
    with open(batch, "w") as f:
        f.write(f"{len(edge)}\n")
        for d in edge:
            f.write(f"{len(d['bases'])} {len(d['hap_bases'])}\n")
            for key in ("bases", "qual", "ins", "dele", "gcp", "hap_bases"):
                f.write(" ".join(str(int(v)) for v in d[key]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, batch], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and not run.stderr, run.stdout[-1000:] + run.stderr[-4000:]
    got = {}
    for ln in run.stdout.splitlines():
        kind, *v = ln.split()
        got[(kind,) + tuple(int(x) for x in v[:-1])] = int(v[-1], 16 if kind == "res" else 10)
    assert len(got) == 5 * len(edge)
    for k, d in enumerate(edge):
        for form in (1, 2, 3, 4):
            res, way = emulate_res(d, form)
            assert got[("res", form, k)] == int(res.view(np.uint32)[0]), (k, form)
        assert got[("way", k)] == int(way[0])
