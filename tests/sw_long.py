"""Inputs of the long-reference Smith-Waterman tests (references of more than 2048 bases, MGX_SW_LONG_REF), regenerated from
seeds wherever they are needed: the oracle test, the GPU tests and tests/golden/make_golden_smithwaterman_long.py."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "smithwaterman_long.npz")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
STANDARD_NGS, ORIGINAL_DEFAULT = (25, -50, -110, -6), (3, -1, -4, -3)
PARAM_SETS = (STANDARD_NGS, ORIGINAL_DEFAULT)
STRATEGIES = (9, 10, 11, 12)          # SOFTCLIP, INDEL, LEADING_INDEL, IGNORE
STRIP_ROWS = 2048                     # 64 lanes x 32 rows: kStripRows of csrc/mgx_smithwaterman.hip

# the shapes the oracle was first compared on, then the seams of 1024 rows (a strip of 16 or of 32 rows per lane ends on them)
SHAPES = [(2049, 1), (2049, 300), (2050, 2050), (4096, 64), (4097, 200), (4160, 513), (6145, 100), (8192, 1000), (3000, 3000),
          (12000, 300), (20000, 150), (32767, 200)]
SEAM_SHAPES = [(k * 1024 + d, m) for k in range(2, 6) for d in (-1, 0, 1) for m in (1, 63, 64, 65, 300)]


def random_bases(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def make_pair(nrow, ncol, seed):
    """a random reference and an alternate that is a piece of it with a 7-base deletion and 2 % substitutions,
    filled up with random bases where the reference is too short for it"""
    rng = np.random.default_rng(seed)
    ref = random_bases(rng, nrow)
    take = min(ncol + 7, nrow)
    start = int(rng.integers(0, nrow - take + 1))
    piece = ref[start:start + take].copy()
    if take >= 30:
        piece = np.concatenate([piece[:take // 2], piece[take // 2 + 7:]])
    mut = rng.random(len(piece)) < 0.02
    piece[mut] = random_bases(rng, int(mut.sum()))
    if len(piece) < ncol:
        piece = np.concatenate([piece, random_bases(rng, ncol - len(piece))])
    return ref, np.ascontiguousarray(piece[:ncol])


def concat(pairs, strategies):
    ro = np.zeros(len(pairs) + 1, dtype=np.uint64); ao = np.zeros(len(pairs) + 1, dtype=np.uint64)
    ro[1:] = np.cumsum([len(r) for r, _ in pairs]); ao[1:] = np.cumsum([len(a) for _, a in pairs])
    return dict(ref_off=ro, ref=np.concatenate([r for r, _ in pairs]), alt_off=ao, alt=np.concatenate([a for _, a in pairs]),
                strategy=np.array(strategies, dtype=np.uint8))


def golden_cases():
    """-> [(ref, alt, params, strategy)] in the order of the fixture: every shape under both parameter sets and all strategies"""
    out = []
    for q, (n, m) in enumerate(SHAPES + SEAM_SHAPES):
        ref, alt = make_pair(n, m, 0x10C0000 + q)
        for params in PARAM_SETS:
            for st in STRATEGIES:
                out.append((ref, alt, params, st))
    return out


def cases_digest(cases):
    h = hashlib.sha256()
    for ref, alt, params, st in cases:
        h.update(np.array(list(params) + [st, len(ref), len(alt)], dtype=np.int64).tobytes())
        h.update(ref.tobytes()); h.update(alt.tobytes())
    return h.hexdigest()


def load_golden(cases):
    """the reference build's (CIGAR texts, offsets) for golden_cases(); refuses a fixture made for other inputs"""
    z = np.load(GOLD)
    assert str(z["inputs_sha256"]) == cases_digest(cases), "smithwaterman_long.npz was not made for these inputs"
    return [bytes(c) for c in z["cigar"]], z["offset"]
