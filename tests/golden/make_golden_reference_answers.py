"""Writes tests/golden/reference_answers.npz: what the reference's own builds (oracle/_ref, see oracle/Makefile) return
for the inputs of the tests that compare the CPU oracles against them.  It runs those tests' bodies with
conftest.RECORD set, so the stored answers belong to exactly the inputs the tests build.
Run in the build container (needs /root/reference for `make -C oracle ref`):
    python tests/golden/make_golden_reference_answers.py"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402


def main():
    for so in ("libref_pairhmm.so", "libref_sortdedup.so", "libref_smithwaterman.so"):
        if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", so)):
            sys.exit("build oracle/_ref first: make -C oracle ref")
    synth = importlib.import_module(conftest.PKG + ".synth")
    oracle = conftest.PairHMMOracle(conftest._ensure_oracle())
    ref_oracle = conftest.PairHMMOracle(os.path.join(ROOT, "oracle", "_ref", "libref_pairhmm.so"), "ref_pairhmm_batch")
    sd_oracle, sd_ref = conftest.SortDedupOracle(), conftest.SortDedupRef(os.path.join(ROOT, "oracle", "_ref", "libref_sortdedup.so"))
    sw_oracle, sw_ref = conftest.SmithWatermanOracle(), conftest.SmithWatermanRef(os.path.join(ROOT, "oracle", "_ref", "libref_smithwaterman.so"))
    import test_pairhmm_oracle as tp
    import test_smithwaterman_oracle as tw
    import test_sortdedup_oracle as ts
    conftest.RECORD = {}
    tp.test_oracle_matches_reference_build_live(oracle, ref_oracle, synth)
    tw.test_oracle_matches_reference_build(sw_oracle, sw_ref, synth)
    tw.test_text_capacity_rule(sw_oracle, sw_ref)
    mark = next(m for m in ts.test_oracle_matches_reference_build_live.pytestmark if m.name == "parametrize")
    for seed, style in mark.args[1]:
        ts.test_oracle_matches_reference_build_live(sd_oracle, sd_ref, synth, seed, style)
    path = os.path.join(HERE, "reference_answers.npz")
    np.savez_compressed(path, **conftest.RECORD)
    print("wrote", path, sorted({k.split("/")[0] for k in conftest.RECORD}), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
