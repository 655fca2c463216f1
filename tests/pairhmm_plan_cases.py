"""Fixed PairHMM batches that the CPU test of the batch plan (test_pairhmm_plan_host.py) and the dispatch comparison recorded in
profiles/pairhmm_plan_refactor_ab.txt share: lengths from a generator of this file's own, so that the plan driver (lengths only) and a
run on the device (make_batch gives the lengths contents; tools/dev_plan_dispatch.py) see the same batch.

FIXED_PAIR_LAUNCHES and FIXED_REGION_LAUNCHES are what the library dispatched for them on an MI355X (256 CUs) BEFORE the plan moved into
csrc/pairhmm_plan.h: the rows of a rocprofv3 --kernel-trace of the parent commit's library running these two batches, in dispatch
order (profiles/pairhmm_plan_refactor_ab.txt section 3).  They are not taken from the header."""
import numpy as np

N_CU = 256


def _lcg(seed):
    s = seed
    while True:
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        yield s >> 33


def fixed_pairs():
    """-> (read lengths, haplotype lengths); test case i is read i against haplotype i.  Every lane width and the strip class occur; two
    16-lane classes hold more than 4096 test cases and keep a launch of their own, the others are folded."""
    g = _lcg(0x5EED0101)
    spec = [(300, 1, 32), (500, 33, 64), (4200, 65, 80), (4100, 113, 128), (700, 129, 192), (400, 193, 1024), (6, 1025, 2600)]
    pairs = []
    for n, lo, hi in spec:
        for _ in range(n):
            r = lo + next(g) % (hi - lo + 1)
            h = 20 + next(g) % 380 if r <= 192 else 100 + next(g) % 900
            pairs.append((r, h))
    for i in range(len(pairs) - 1, 0, -1):          # Fisher-Yates: the classes arrive interleaved
        j = next(g) % (i + 1)
        pairs[i], pairs[j] = pairs[j], pairs[i]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def fixed_regions():
    """-> [(read lengths, haplotype lengths)] of six regions in the cross-product form, one of them a single test case"""
    g = _lcg(0x5EED0202)
    shapes = [(24, 16, (20, 128), (64, 256)), (1, 1, (100, 100), (200, 200)), (40, 25, (90, 151), (150, 400)),
              (7, 3, (200, 400), (300, 600)), (60, 9, (30, 60), (40, 90)), (3, 40, (151, 151), (200, 300))]
    out = []
    for nr, nh, (r0, r1), (h0, h1) in shapes:
        out.append(([r0 + next(g) % (r1 - r0 + 1) for _ in range(nr)], [h0 + next(g) % (h1 - h0 + 1) for _ in range(nh)]))
    return out


def make_batch(rlens, hlens, seed, pairs=True):
    """the packed dict PairHMMEngine takes, with random contents of the given lengths (pairs: test case i = read i x haplotype i;
    otherwise the cross-product form)"""
    rng = np.random.default_rng(seed)
    rb, hb = int(sum(rlens)), int(sum(hlens))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    d = dict(read_off=np.concatenate([[0], np.cumsum(rlens)]).astype(np.uint64), hap_off=np.concatenate([[0], np.cumsum(hlens)]).astype(np.uint64),
             bases=letters[rng.integers(0, 4, rb)], hap_bases=letters[rng.integers(0, 4, hb)],
             qual=rng.integers(6, 42, rb).astype(np.uint8), ins=rng.integers(10, 46, rb).astype(np.uint8),
             dele=rng.integers(10, 46, rb).astype(np.uint8), gcp=np.full(rb, 10, dtype=np.uint8))
    if pairs:
        d["pair_read"] = np.arange(len(rlens), dtype=np.uint32)
        d["pair_hap"] = np.arange(len(hlens), dtype=np.uint32)
    else:
        d["pair_read"] = d["pair_hap"] = None
    return d


# (kernel, G, RPL, code columns, workgroups, workgroup size, dynamic LDS bytes) in dispatch order on the compute stream; kernel:
# "multi" (G = GSET), "f32", "f64", "strip32", "strip64", "exact".  Kernel, workgroups and workgroup size are the trace's rows.  The
# trace's LDS_Block_Size column read 0 for these launches, so the LDS bytes were recorded in a second run of the same script on a
# scratch build of the parent commit whose launch sites print their grid, block and LDS argument (same order, same grids).
FIXED_PAIR_LAUNCHES = [
    ('multi', 0, 0, 4, 2075, 64, 9984), ('multi', 1, 0, 4, 82, 64, 14848), ('f32', 64, 16, 4, 400, 64, 17520),
    ('f32', 64, 16, 5, 400, 64, 21616), ('f64', 64, 16, 5, 400, 64, 1136), ('f32', 16, 8, 5, 1025, 64, 12032),
    ('f32', 16, 5, 5, 1050, 64, 9472), ('f32', 16, 12, 4, 175, 64, 14464), ('f32', 16, 12, 5, 175, 64, 17536),
    ('f64', 64, 3, 5, 700, 64, 544), ('strip32', 64, 16, 5, 6, 64, 21488), ('strip64', 64, 16, 5, 6, 64, 1008),
    ('f32', 8, 8, 5, 63, 64, 13696), ('f32', 4, 8, 5, 19, 64, 16896), ('f64', 16, 8, 5, 2048, 64, 1792),
    ('exact', 64, 16, 5, 512, 64, 1136),
]
FIXED_REGION_LAUNCHES = [
    ('multi', 1, 0, 4, 90, 64, 15616), ('f32', 16, 12, 4, 321, 64, 14656), ('f32', 16, 12, 5, 321, 64, 17728),
    ('f64', 64, 3, 5, 1281, 64, 592), ('f32', 64, 16, 4, 21, 64, 16976), ('f32', 64, 16, 5, 21, 64, 21072),
    ('f64', 64, 16, 5, 21, 64, 592), ('f32', 8, 8, 5, 83, 64, 14080), ('f32', 4, 8, 5, 7, 64, 17664),
    ('f64', 16, 4, 5, 191, 64, 1984), ('exact', 64, 16, 5, 512, 64, 592),
]
