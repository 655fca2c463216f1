"""Inputs shared by the tests of the PairHMM wire form (csrc/pairhmm_wire.h): streams crafted so that reads start at every
position of a group of eight in the 6- and 7-bit streams and at both nibble phases, the width-selection cases, the base-folding cases, and the
canonical form that an expanded batch must equal."""
import itertools

import numpy as np

SEAM_LENGTHS = (1, 7, 8, 9, 15, 16, 17)
_FOLD = np.full(256, ord("A"), dtype=np.uint8)
for _c in b"ACTGN":
    _FOLD[_c] = _c
ARRAYS = ("bases", "qual", "ins", "dele", "gcp", "hap_bases")


def canonical(p):
    """What expansion must give for the packed batch ``p`` (pack_batch's dict): qualities masked with 127, bases folded to
    A C T G N; offsets and pair arrays as they are."""
    c = dict(p)
    for k in ("qual", "ins", "dele", "gcp"):
        c[k] = p[k] & np.uint8(127)
    c["bases"] = _FOLD[p["bases"]]
    c["hap_bases"] = _FOLD[p["hap_bases"]]
    return c


def assert_same_batch(got, want, what=""):
    for k in ("n_reads", "n_haps", "n_pairs"):
        assert got[k] == want[k], (what, k)
    for k in ("read_off", "hap_off", "pair_read", "pair_hap") + ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def stream(read_lens, hap_lens, pairs=None, seed=0, qmax=63, gcp=10):
    """A pair-list stream with the given sequence lengths; qualities uniform in [0, qmax], one gcp value.  Default test
    cases: i -> (read i % nr, haplotype i % nh) for i < max(nr, nh), which uses every sequence, in order."""
    rng = np.random.RandomState(seed)
    nr, nh = len(read_lens), len(hap_lens)
    rb, hb = int(sum(read_lens)), int(sum(hap_lens))
    if pairs is None:
        pairs = [(i % nr, i % nh) for i in range(max(nr, nh))]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    d = dict(read_off=np.concatenate([[0], np.cumsum(read_lens)]).astype(np.uint64),
             hap_off=np.concatenate([[0], np.cumsum(hap_lens)]).astype(np.uint64),
             bases=acgt[rng.randint(0, 4, rb)], hap_bases=acgt[rng.randint(0, 4, hb)],
             qual=rng.randint(0, qmax + 1, rb).astype(np.uint8), ins=rng.randint(0, qmax + 1, rb).astype(np.uint8),
             dele=rng.randint(0, qmax + 1, rb).astype(np.uint8), gcp=np.full(rb, gcp, dtype=np.uint8),
             pair_read=np.array([p[0] for p in pairs], dtype=np.uint32), pair_hap=np.array([p[1] for p in pairs], dtype=np.uint32))
    d["n_reads"], d["n_haps"], d["n_pairs"] = nr, nh, len(pairs)
    return d


def seam_stream(seed=1):
    """the seven seam lengths as reads (7-bit qualities in `qual`, 6-bit in `ins` / `dele`, a varying gcp), odd haplotypes"""
    d = stream(SEAM_LENGTHS, (1, 3, 5, 2, 9, 33, 7), seed=seed)
    rng = np.random.RandomState(seed + 100)
    d["qual"] = rng.randint(0, 128, len(d["qual"])).astype(np.uint8)
    d["gcp"] = rng.randint(0, 64, len(d["gcp"])).astype(np.uint8)
    return d


def seam_orders(every=True):
    """orders of the seven seam reads: all 5040, or the rotations, the reversal and a few more"""
    if every:
        return list(itertools.permutations(range(7)))
    rot = [tuple((i + s) % 7 for i in range(7)) for s in range(7)]
    return rot + [tuple(reversed(range(7))), (3, 0, 6, 1, 5, 2, 4), (6, 4, 2, 0, 5, 3, 1), (1, 0, 3, 2, 5, 4, 6)]


def with_order(d, order):
    """the same stream with its test cases in `order`: the packer gathers the reads in first-use order"""
    e = dict(d)
    e["pair_read"] = np.array(order, dtype=np.uint32)
    e["pair_hap"] = np.array(order, dtype=np.uint32) % np.uint32(len(d["hap_off"]) - 1)
    e["n_pairs"] = len(order)
    return e


def small_shapes():
    """name -> stream: total read bases of 1, 7, 8 and 9, haplotypes of 1 and of odd length, one read or one haplotype only"""
    out = {}
    for n in (1, 7, 8, 9):
        out[f"one_read_{n}"] = stream((n,), (1,), seed=n)
        out[f"one_read_{n}_q7"] = stream((n,), (3,), seed=n, qmax=127)
    out["reads_3_4"] = stream((3, 4), (5, 1), seed=11)
    out["reads_1_x9"] = stream((1,) * 9, (7,), seed=12)                     # one haplotype only
    out["one_read_many_haps"] = stream((13,), (1, 1, 3, 255, 2), seed=13)   # one read only
    out["reads_3_x9"] = stream((3,) * 9, (4, 9), seed=15, qmax=127)         # with the next: reads start at every phase of a group
    out["reads_5_x9"] = stream((5,) * 9, (4, 9), seed=16)
    out["odd_haps"] = stream((16, 8), (1, 31, 257), seed=14, qmax=127)
    return out


def width_cases():
    """[(name, stream, expected dict of w_qual / w_ins / w_del / w_gcp and gcp_const where it applies)]; every array is varied on
    its own while the others stay at 6 bits and a constant gcp"""
    base = stream((5, 16, 20, 9), (12, 7), seed=21)             # 50 read bases: the last partial group holds positions 48 and 49
    rb = len(base["qual"])
    six = dict(w_qual=6, w_ins=6, w_del=6, w_gcp=0, gcp_const=10)
    cases = [("all_6", base, six)]

    def put(arr, pos, val, name, **expect):
        d = dict(base)
        d[arr] = base[arr].copy()
        d[arr][pos] = val
        cases.append((name, d, dict(six, **expect)))
    key = {"qual": "w_qual", "ins": "w_ins", "dele": "w_del"}
    for arr, wk in key.items():
        put(arr, 0, 64, f"{arr}_64_first", **{wk: 7})
        put(arr, rb - 1, 64, f"{arr}_64_last", **{wk: 7})
        put(arr, 48, 64, f"{arr}_64_last_group", **{wk: 7})
        put(arr, 17, 127, f"{arr}_127", **{wk: 7})
        put(arr, slice(None), base[arr] | 128, f"{arr}_high_bit_set")          # masked values still <= 63
        put(arr, 23, 0, f"{arr}_zero")
        put(arr, 23, 255, f"{arr}_255", **{wk: 7})
    mixed = np.where(np.arange(rb) % 3 == 0, 138, 10).astype(np.uint8)
    put("gcp", slice(None), mixed, "gcp_10_and_138")                            # one value after the mask
    put("gcp", 31, 11, "gcp_one_differs", w_gcp=6)
    put("gcp", 31, 64, "gcp_one_64", w_gcp=7)
    put("gcp", 49, 0, "gcp_zero_last", w_gcp=6)                                  # the byte of 0 the kernels' plain form looks for
    put("gcp", slice(None), 0, "gcp_all_zero", gcp_const=0)
    put("gcp", slice(None), 127 | 128, "gcp_all_255", gcp_const=127)
    return cases


def base_cases():
    """streams whose bases hold lower case, IUPAC letters, 0x00 and 0xFF (all expand to A) and N (stays N)"""
    d = stream((9, 6, 11), (13, 4), seed=31)
    odd = np.frombuffer(b"acgtnRYKMSWBDHVU\x00\xff.-*NNAN", dtype=np.uint8)
    e = dict(d)
    e["bases"] = np.resize(odd, len(d["bases"]))
    e["hap_bases"] = np.resize(odd[::-1], len(d["hap_bases"]))
    every = stream((256,), (256,), seed=32)
    every["bases"] = np.arange(256, dtype=np.uint8)
    every["hap_bases"] = np.arange(256, dtype=np.uint8)[::-1].copy()
    return {"mixed": e, "every_byte": every}


def crafted():
    """name -> stream: everything above but the 5040 orders, for the tests that run each case once"""
    out = dict(small_shapes())
    seam = seam_stream()
    for order in seam_orders(every=False):
        out["seam_" + "".join(map(str, order))] = with_order(seam, order)
    for name, d, _ in width_cases():
        out["width_" + name] = d
    for name, d in base_cases().items():
        out["bases_" + name] = d
    return out


def concat_streams(a, b):
    """two pair-list streams as one"""
    nra, nha = len(a["read_off"]) - 1, len(a["hap_off"]) - 1
    d = {k: np.concatenate([a[k], b[k]]) for k in ARRAYS}
    d["read_off"] = np.concatenate([a["read_off"], b["read_off"][1:] + a["read_off"][-1]]).astype(np.uint64)
    d["hap_off"] = np.concatenate([a["hap_off"], b["hap_off"][1:] + a["hap_off"][-1]]).astype(np.uint64)
    d["pair_read"] = np.concatenate([a["pair_read"], b["pair_read"] + np.uint32(nra)]).astype(np.uint32)
    d["pair_hap"] = np.concatenate([a["pair_hap"], b["pair_hap"] + np.uint32(nha)]).astype(np.uint32)
    return d


def ragged_with_everything(synth, n=4000, seed=0x5EED0010, zero_gcp_in_short_reads=True):
    """`n` ragged test cases that reach every launch the expanded arrays feed: haplotypes with N (the five-code launch), reads
    with a gap-continuation byte of 0 (the plain form), quality bytes >= 128, one read of 1 100 bases (the strip-mined class),
    and random reads whose likelihood underflows fp32 (the fp64 re-run).

    A wavefront that sees a gap-continuation byte of 0 takes the plain form for every test case it holds
    (pairhmm_kernels.hip.inc, above `use_plain`).  With such bytes in short reads, which share wavefronts, a plain queue run
    twice on this stream did not compare equal to itself under np.array_equal (a NaN among the results; 23 of 4 000 values
    differed between per-batch and whole-stream runs of a plain engine), so no bit-for-bit yardstick exists there.
    zero_gcp_in_short_reads=False, which the tests use, puts the zero bytes into twelve reads of 200-400 bases only: those
    classes run one test case per wavefront."""
    n_long = 12
    a = synth.gen_pairhmm_pairs(n - 1 - n_long, seed, r_range=(1, 130), h_range=(10, 260), hap_n_rate=0.004, random_read_rate=1 / 64)
    b = synth.gen_pairhmm_pairs(1, seed + 1, r_range=(1100, 1100), h_range=(1300, 1300))
    c = synth.gen_pairhmm_pairs(n_long, seed + 2, r_range=(200, 400), h_range=(300, 500))
    d = concat_streams(concat_streams(a, c), b)
    rng = np.random.RandomState(5)
    ro = d["read_off"].astype(np.int64)
    short = rng.choice(n - 1 - n_long, 60, replace=False) if zero_gcp_in_short_reads else []
    for r in list(short) + list(range(n - 1 - n_long, n - 1)):      # whole reads and single positions with gcp 0
        if r % 2:
            d["gcp"][ro[r]:ro[r + 1]] = 0
        else:
            d["gcp"][ro[r] + (ro[r + 1] - ro[r]) // 2] = 0
    for k in ("qual", "ins", "dele", "gcp"):                    # bit 7 carries nothing: the kernels mask it
        d[k] = np.where(rng.randint(0, 16, len(d[k])) == 0, d[k] | np.uint8(128), d[k]).astype(np.uint8)
    d["ins"] = np.where(rng.randint(0, 8, len(d["ins"])) == 0, d["ins"] + np.uint8(40), d["ins"]).astype(np.uint8)      # up to 85: a 7-bit array
    order = rng.permutation(n)                                   # the long reads somewhere in the middle
    d["pair_read"] = d["pair_read"][order]; d["pair_hap"] = d["pair_hap"][order]
    return d
