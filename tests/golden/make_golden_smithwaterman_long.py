"""Generates tests/golden/smithwaterman_long.npz from the REFERENCE's own aligner compiled in place
(oracle/_ref/libref_smithwaterman.so, see oracle/Makefile): its CIGAR text and offset for references of more than 2048 bases.
The inputs are regenerated from seeds (tests/sw_long.py); the file holds their digest and the answers, not the sequences.
Run where the reference tree is present (`make -C oracle ref`)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import SmithWatermanRef  # noqa: E402
import sw_long  # noqa: E402

ref = SmithWatermanRef(os.path.join(ROOT, "oracle", "_ref", "libref_smithwaterman.so"))
cases = sw_long.golden_cases()
cig, off = [], []
for r, a, params, st in cases:
    c, o = ref.align(r, a, params, st)
    cig.append(c); off.append(o)
np.savez_compressed(sw_long.GOLD, inputs_sha256=np.array(sw_long.cases_digest(cases)), cigar=np.array(cig, dtype=np.bytes_),
                    offset=np.array(off, dtype=np.int32))
print("wrote", sw_long.GOLD, len(cases), "pairs,", os.path.getsize(sw_long.GOLD), "bytes")
