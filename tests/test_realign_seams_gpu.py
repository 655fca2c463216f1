"""mgx_realign_regions and mgx_realign_regions_to_ref (csrc/mgx_realign.hip) where the two contexts join, in the configurations the
other realign tests never take: several aligner chunks, every fill family behind the gather, the threaded text stage with the element
sink attached, every overhang strategy and other score parameters, the gather's event pair across chunks, regions that are views into
larger arrays and regions without haplotypes.  Every comparison is exact (bytes, integers, CIGAR text).

Every region is built from a plan (class Plan): each read is cut from a haplotype the plan knows and is meant to be dropped, found
verbatim or aligned.  What a call must have done -- which reads reach the aligner, how long its pairs are, where the chunks are cut --
is therefore known on the CPU before the device runs (the cuts through the layout driver of test_sw_layout_host.py), and every test
asserts from that side that it reached its seam; the device's keep flags and best haplotypes must then equal the plan's.

The read model decides what is kept (read_model_cases.restated_normalize_filter): a read of more than 50 bases is dropped below
log10 -8, a shorter one below -4.  A read of constant quality 30 that matches its haplotype scores about -log10(haplotype length);
a Q30 substitution costs 3.5, a one-base gap at gap quality 30 costs 3, a base with MAPQ 0 (quality 6) costs 0.126.  So the plans cut
edited reads of 60 bases or more and dropped reads of 80 or more (or say why theirs are safe)."""
import numpy as np
import pytest

import read_to_ref_cases as C
import realign_cases as RC
import sw_frontier as F
from read_model_cases import _subview
from test_read_to_ref_gpu import check_to_ref_of_regions, to_ref_part
from test_realign_gpu import check_against_composer, gather_region, make_region, other, seq
from test_sw_layout_host import LayoutDriver

pytestmark = pytest.mark.gpu
KNOBS = ("MGX_SW_ARENA_LIMIT", "MGX_SW_I16", "MGX_SW_PAIRED")
COUNTERS = ("n_reads", "n_kept", "n_verbatim", "n_sw_pairs")
SHORTCUT = (RC.SOFTCLIP, RC.IGNORE)
MIB = 1 << 20
PAIRED_FROM, THREADED_FROM = 8192, 16384        # sw_layout.h kPairedFrom; emit_text's k.n >= 16384 in mgx_smithwaterman.hip


# ---- plans ------------------------------------------------------------------------------------------------------------------------
class Plan:
    """One region under construction: random haplotypes, and per read (bases, kind, haplotype it was cut from, low-quality bases at
    its front and back).  kind: "verbatim" (kept, occurs in its haplotype), "dropped" (verbatim, MAPQ 0), anything else: kept and
    not a substring of its haplotype, so it needs the aligner under every strategy."""

    def __init__(self, rng, hap_lens):
        self.rng, self.haps, self.reads, self.low_at = rng, [seq(rng, int(n)) for n in hap_lens], [], {}       # low_at: read -> its edit, of quality 10

    def add(self, kind, h, bases, low=(0, 0)):
        found = RC.last_index_of(self.haps[h], bases) >= 0
        assert found == (kind in ("verbatim", "dropped")), (kind, h, bases)
        self.reads.append((bytes(bases), kind, h, low))

    def cut(self, kind, h, R, low_at_edit=False):
        """a read of R bases out of haplotype h; "sub", "del", "ins": one edit at least 8 bases from either end"""
        hap, rng = self.haps[h], self.rng
        at, p = int(rng.randint(0, len(hap) - R)), int(rng.randint(8, R - 8)) if R >= 17 else R // 2
        if kind in ("verbatim", "dropped"):
            new = hap[at:at + R]
        elif kind == "sub":
            new = hap[at:at + p] + other(hap[at + p]) + hap[at + p + 1:at + R]
        elif kind == "del":
            new = hap[at:at + p] + hap[at + p + 1:at + R + 1]
        else:
            new = hap[at:at + p] + other(hap[at + p]) + hap[at + p:at + R - 1]
        assert len(new) == R
        self.add(kind, h, new)
        if low_at_edit:
            self.low_at[len(self.reads) - 1] = p

    def region(self):
        """-> (region dict, mapq): quality 30, gap qualities 30; the low ends and the marked edits get quality 10, the low ends an
        insertion quality of 10 as well"""
        d = make_region(self.haps, [b for b, _, _, _ in self.reads])
        d["ins"][:] = 30; d["dele"][:] = 30
        ro = d["read_off"].astype(np.int64)
        for r, (_, _, _, (front, back)) in enumerate(self.reads):
            for lo, hi in ((ro[r], ro[r] + front), (ro[r + 1] - back, ro[r + 1])):
                d["qual"][lo:hi] = 10; d["ins"][lo:hi] = 10
        for r, p in self.low_at.items():
            d["qual"][ro[r] + p] = 10
        return d, np.array([0 if kind == "dropped" else 60 for _, kind, _, _ in self.reads], dtype=np.uint8)

    def keep(self):
        return [int(kind != "dropped") for _, kind, _, _ in self.reads]

    def pairs(self, strategy):
        """(haplotype, read) of the reads the aligner gets, in read order"""
        return [(self.haps[h], b) for b, kind, h, _ in self.reads if kind != "dropped" and not (kind == "verbatim" and strategy in SHORTCUT)]

    def n_verbatim(self, strategy):
        return sum(kind == "verbatim" for _, kind, _, _ in self.reads) if strategy in SHORTCUT else 0


def pair_lens(plans, strategy=RC.SOFTCLIP):
    return [(len(hap), len(read)) for p in plans for hap, read in p.pairs(strategy)]


def check_plan(plans, res, realign, strategy=RC.SOFTCLIP):
    """the device kept, and found best, what the plans say; with that the counters are the plans' too"""
    for g, (p, o) in enumerate(zip(plans, res)):
        assert list(o["keep"]) == p.keep(), (g, [r for r, (a, b) in enumerate(zip(o["keep"], p.keep())) if a != b][:5])
        bad = [(r, int(o["best"][r]), h) for r, (_, kind, h, _) in enumerate(p.reads) if kind != "dropped" and o["best"][r] != h]
        assert not bad, (g, bad[:5])
    st = realign.stats()
    n_pairs = len(pair_lens(plans, strategy))
    want = (sum(len(p.reads) for p in plans), sum(sum(p.keep()) for p in plans), sum(p.n_verbatim(strategy) for p in plans), n_pairs)
    assert tuple(st[k] for k in COUNTERS) == want, (st, want)
    return st


def assert_same(got, want, to_ref=False):
    """every output array of two calls, byte for byte"""
    assert len(got) == len(want)
    for g, (o, w) in enumerate(zip(got, want)):
        for k in ("log10", "keep", "best", "offset", "score") + (("start", "status", "n_ref_cigar") if to_ref else ()):
            assert o[k].shape == w[k].shape and o[k].tobytes() == w[k].tobytes(), (g, k)
        assert o["cigar"] == w["cigar"], (g, [(r, a, b) for r, (a, b) in enumerate(zip(o["cigar"], w["cigar"])) if a != b][:3])
        if to_ref:
            assert len(o["ref_cigar"]) == len(w["ref_cigar"]) and all(np.array_equal(a, b) for a, b in zip(o["ref_cigar"], w["ref_cigar"])), g


def counters(realign):
    st = realign.stats()
    return tuple(st[k] for k in COUNTERS)


def status_counts(res):
    n = [0] * 6
    for o in res:
        for s in o["status"]:
            n[int(s)] += 1
    return n


@pytest.fixture(scope="module")
def realign(pkg, engine, sw_engine):
    return pkg.RealignEngine(engine, sw_engine)


@pytest.fixture(scope="module")
def cuts_of(tmp_path_factory):
    """(pair lengths, arena limit, knobs) -> [(lo, hi, back-trace bytes)]: chunk_end and build_jobs of csrc/sw_layout.h on the CPU"""
    driver = LayoutDriver(tmp_path_factory.mktemp("realign_seams_layout"), sanitize=False)

    def cuts(lens, limit, params=RC.TO_BEST_HAPLOTYPE, strategy=RC.SOFTCLIP, paired=0, use16=1):
        res = driver.run(lens, strategies=[strategy] * len(lens), params=params, paired=paired, use16=use16, limit=limit)
        return [(lo, hi, arena) for lo, hi, _, arena, _ in res["cuts"]]
    return cuts


class Batch:
    def __init__(self, plans, rng, hard=True):
        self.plans = plans
        self.regions, self.mapqs = [list(x) for x in zip(*(p.region() for p in plans))]
        self.to_ref = to_ref_part(self.regions, rng, hard=hard)
        self.lens = pair_lens(plans)


def mixed_plan(rng, hap_lens, n_reads, aligned=(140, 151)):
    """reads in the order sub, del, verbatim, ins, dropped, sub, ...: four of six need the aligner, and those are 140-150 bases long"""
    p = Plan(rng, hap_lens)
    for r in range(n_reads):
        kind, h = ("sub", "del", "verbatim", "ins", "dropped", "sub")[r % 6], int(rng.randint(len(hap_lens)))
        R = {"verbatim": rng.randint(20, 151), "dropped": rng.randint(80, 151)}.get(kind, rng.randint(*aligned))
        p.cut(kind, h, min(int(R), int(hap_lens[h]) - 2))
    return p


def make_batch():
    """three regions of 2, 5 and 3 haplotypes of 240-299 bases, 24 reads each: 48 aligner pairs of about 260 x 145 bases"""
    rng = np.random.RandomState(41)
    b = Batch([mixed_plan(rng, rng.randint(240, 300, nh), 24) for nh in (2, 5, 3)], rng)
    b.to_ref[1]["ref_hap"] = 1
    assert len(b.lens) == 48 and all(l1 >= 240 and l2 >= 140 for l1, l2 in b.lens)
    # a haplotype -> reference CIGAR with an insertion and a deletion under a kept read, hard clips on some reads
    used = {(g, h) for g, p in enumerate(b.plans) for _, kind, h, _ in p.reads if kind != "dropped"}
    assert any({1, 2} <= {int(e) & 15 for e in b.to_ref[g]["hap_cigars"][h]} for g, h in used)
    assert any(t["hard_clips"].any() for t in b.to_ref)
    return b


@pytest.fixture(scope="module")
def batch():
    return make_batch()


@pytest.fixture(scope="module")
def reference(realign, batch, sw_oracle):
    """the batch in one chunk under the default knobs, checked against the composer and the restatement once; the other tests compare
    with it byte for byte"""
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        res = realign.regions(batch.regions, batch.mapqs)
        st = check_plan(batch.plans, res, realign)
        assert realign.sw.stats()["n_launches"] >= 1
        fused = realign.regions_to_ref(batch.regions, batch.mapqs, batch.to_ref, ref_stride=16)
        n_status = realign.to_ref_stats()["n_status"]
    assert check_against_composer(sw_oracle, batch.regions, res) == st["n_verbatim"] > 0
    assert_same(fused, res)
    seen = check_to_ref_of_regions(batch.regions, batch.to_ref, fused, 16)
    assert n_status == [seen.get(s, 0) for s in range(6)] and seen[C.DROPPED] == 12 and seen.get(C.OK, 0) > 0, seen
    return dict(res=res, fused=fused, counters=tuple(st[k] for k in COUNTERS), n_status=n_status)


# ---- 1. several chunks ------------------------------------------------------------------------------------------------------------
def test_several_aligner_chunks_under_both_calls(realign, batch, reference, sw_oracle, cuts_of, monkeypatch):
    """Gap "aligner chunks": MGX_SW_ARENA_LIMIT = 1 MiB cuts the 48 pairs into chunks, so gather_chunk runs with lo > 0
    (gjobs.dev + lo, base_ref = ref_off[lo], base_alt = alt_off[lo]), the element sink's offsets carry over from chunk to chunk and
    to_ref_stage reads them by the global pair index.  Reached: the cuts come from chunk_end on the CPU, and the device's
    back-trace bytes are the sum over exactly those chunks' layouts."""
    cuts = cuts_of(batch.lens, MIB)
    assert len(cuts) >= 4 and cuts[-1][1] == len(batch.lens) and all(lo > 0 for lo, _, _ in cuts[1:])
    monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(MIB))
    res = realign.regions(batch.regions, batch.mapqs)
    sw_stats = realign.sw.stats()
    assert sw_stats["n_launches"] >= len(cuts) and sw_stats["backtrace_bytes"] == sum(a for _, _, a in cuts), (sw_stats, cuts)
    assert sw_stats["n_pairs"] == len(batch.lens)
    check_plan(batch.plans, res, realign)
    assert counters(realign) == reference["counters"]
    assert check_against_composer(sw_oracle, batch.regions, res) == reference["counters"][2]
    assert_same(res, reference["res"])
    fused = realign.regions_to_ref(batch.regions, batch.mapqs, batch.to_ref, ref_stride=16)
    assert realign.sw.stats()["backtrace_bytes"] == sum(a for _, _, a in cuts)
    assert counters(realign) == reference["counters"] and realign.to_ref_stats()["n_status"] == reference["n_status"]
    check_to_ref_of_regions(batch.regions, batch.to_ref, fused, 16)
    assert_same(fused, reference["fused"], to_ref=True)
    assert sum(any((int(e) & 15) in (1, 2) for e in c) for o in fused for c in o["ref_cigar"]) > 0


def make_growing_batch():
    """four regions whose 11 aligner pairs get longer along the batch, each with lengths of its own"""
    rng = np.random.RandomState(43)
    plans = []
    for g, (nh, hap_len, Rs) in enumerate(((2, 64, (60, 61)), (3, 130, (90, 100, 110)), (1, 210, (120, 130)), (4, 299, (140, 145, 150, 150)))):
        p = Plan(rng, [hap_len + 3 * k for k in range(nh)])
        for k, R in enumerate(Rs):
            p.cut(("sub", "ins", "del")[(g + k) % 3], k % nh, R)
            if k == 0:
                p.cut("verbatim", nh - 1, 30 + g)
                p.cut("dropped", 0, hap_len - 1 if hap_len < 100 else 100)    # 63 bases of quality 6: -7.9 - 1.8, below -8
        plans.append(p)
    b = Batch(plans, rng)
    n = len(b.lens)
    assert n == 11 and len({x for x in b.lens}) == n                          # every pair of lengths of its own
    first = lambda k: (b.lens[0][k] + 16) + (b.lens[0][k] + 16) // 4 + 64  # noqa: E731
    assert any(l1 + 16 > first(0) for l1, _ in b.lens[1:]) and any(l2 + 16 > first(1) for _, l2 in b.lens[1:])
    return b


def test_one_pair_per_chunk_with_growing_sequence_arrays(pkg, engine, sw_oracle, cuts_of, monkeypatch):
    """Gap "aligner chunks", every value of lo: MGX_SW_ARENA_LIMIT = 1 leaves one pair per chunk (chunk_end takes one at the least).
    The pairs get longer along the batch and the aligner context is new, so d_s1 / d_s2 are reserved again between chunks: a later
    pair exceeds what the first reservation (a quarter and 64 bytes over what was asked) holds."""
    b = make_growing_batch()
    plans, n = b.plans, len(b.lens)
    cuts = cuts_of(b.lens, 1)
    assert [(lo, hi) for lo, hi, _ in cuts] == [(q, q + 1) for q in range(n)]
    sw, plain = pkg.SmithWatermanEngine(0), None
    try:
        realign = pkg.RealignEngine(engine, sw)
        monkeypatch.setenv("MGX_SW_ARENA_LIMIT", "1")
        res = realign.regions(b.regions, b.mapqs)
        st = sw.stats()
        assert st["n_launches"] >= n and st["backtrace_bytes"] == sum(a for _, _, a in cuts) and st["n_pairs"] == n
        check_plan(plans, res, realign)
        fused = realign.regions_to_ref(b.regions, b.mapqs, b.to_ref, ref_stride=16)
        n_status = realign.to_ref_stats()["n_status"]
        monkeypatch.delenv("MGX_SW_ARENA_LIMIT")
        plain = realign.regions_to_ref(b.regions, b.mapqs, b.to_ref, ref_stride=16)
        assert sw.stats()["backtrace_bytes"] == cuts_of(b.lens, 1 << 40)[0][2]        # ... and this one was one chunk
        assert realign.to_ref_stats()["n_status"] == n_status
    finally:
        sw.close()
    check_against_composer(sw_oracle, b.regions, res)
    assert_same(fused, res)
    assert_same(fused, plain, to_ref=True)
    seen = check_to_ref_of_regions(b.regions, b.to_ref, fused, 16)
    assert n_status == [seen.get(s, 0) for s in range(6)] and seen[C.DROPPED] == 4


# ---- 2. timing --------------------------------------------------------------------------------------------------------------------
def test_the_gather_is_timed_across_chunks(pkg, sw_engine, batch, reference, cuts_of, monkeypatch):
    """Gap "MGX_PAIRHMM_TIMING": the event pair ev[3] / ev[4] is recorded once per chunk and read one chunk late (GatherCtx::pending);
    with the flag every output must stay what it is without, the four times must be there, and a call without aligner pairs must not
    show the gather time of the call before it.  No magnitudes."""
    n_chunks = len(cuts_of(batch.lens, MIB))
    assert n_chunks >= 4
    timed = pkg.PairHMMEngine(0, flags=2)                                     # MGX_PAIRHMM_TIMING
    try:
        realign = pkg.RealignEngine(timed, sw_engine)
        monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(MIB))
        res = realign.regions(batch.regions, batch.mapqs)
        st = realign.stats()
        assert sw_engine.stats()["n_launches"] >= n_chunks
        assert_same(res, reference["res"])
        assert tuple(st[k] for k in COUNTERS) == reference["counters"]
        assert st["ms_best"] > 0 and st["ms_verbatim"] > 0 and st["ms_gather"] > 0, st
        fused = realign.regions_to_ref(batch.regions, batch.mapqs, batch.to_ref, ref_stride=16)
        st = realign.stats()
        assert_same(fused, reference["fused"], to_ref=True)
        assert st["ms_best"] > 0 and st["ms_verbatim"] > 0 and st["ms_gather"] > 0 and realign.to_ref_stats()["ms_to_ref"] > 0, st
        assert realign.to_ref_stats()["n_status"] == reference["n_status"]
        # every read verbatim: no aligner pair, no gather
        d, mapq = gather_region(np.random.RandomState(17), (), True)
        res = realign.regions([d], [mapq])
        st = realign.stats()
        assert list(res[0]["keep"]) == [1] * 7 and (st["n_verbatim"], st["n_sw_pairs"]) == (7, 0)
        assert st["ms_gather"] == 0 and st["ms_best"] > 0 and st["ms_verbatim"] > 0, st
    finally:
        timed.close()


# ---- 3. fill families -------------------------------------------------------------------------------------------------------------
def make_batch_with_a_long_haplotype(batch):
    """the batch with a region between its first and second whose only haplotype has 2049 bases (-3.3 for its length)"""
    rng = np.random.RandomState(47)
    long_plan = Plan(rng, [2049])
    long_plan.cut("sub", 0, 120); long_plan.cut("verbatim", 0, 100); long_plan.cut("dropped", 0, 150)
    return Batch(batch.plans[:1] + [long_plan] + batch.plans[1:], rng)


def test_every_fill_family_behind_the_gather(pkg, engine, realign, batch, reference, sw_oracle, cuts_of, monkeypatch):
    """Gap "fill families": MGX_SW_I16 x MGX_SW_PAIRED (read per call) on the gathered sequences, in one chunk and in chunks of 1 MiB,
    and a best haplotype of 2049 bases (a strip-mined pair, LONG_REF context) between ordinary regions of a chunked call.  The
    results are the composer's and the same under all four settings; the 16-bit family ran exactly where it was asked for."""
    with_long = make_batch_with_a_long_haplotype(batch)
    plans = with_long.plans
    strip = [q for q, (l1, _) in enumerate(with_long.lens) if l1 > 2048]
    assert len(strip) == 1 and 0 < strip[0] < len(with_long.lens) - 1
    n_chunks = len(cuts_of(batch.lens, MIB))
    long_cuts = cuts_of(with_long.lens, MIB)
    assert n_chunks >= 4 and len(long_cuts) >= 4
    assert any(lo <= strip[0] < hi and hi - lo > 1 for lo, hi, _ in long_cuts)                  # ordinary pairs in the strip-mined pair's chunk
    long_sw = pkg.SmithWatermanEngine(0, pkg.smithwaterman.LONG_REF)
    try:
        long_realign = pkg.RealignEngine(engine, long_sw)
        first_long = None
        for i16 in (1, 0):
            for paired in (0, 1):
                monkeypatch.setenv("MGX_SW_I16", str(i16)); monkeypatch.setenv("MGX_SW_PAIRED", str(paired))
                for limit in (None, MIB):
                    if limit is None:
                        monkeypatch.delenv("MGX_SW_ARENA_LIMIT", raising=False)
                    else:
                        monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(limit))
                    res = realign.regions(batch.regions, batch.mapqs)
                    where = (i16, paired, limit)
                    st, sw_stats = realign.stats(), realign.sw.stats()
                    assert sw_stats["n_pairs"] == st["n_sw_pairs"] == len(batch.lens), where
                    assert (sw_stats["n_pairs_i16"] > 0) == bool(i16), (where, sw_stats)
                    assert sw_stats["n_launches"] >= (n_chunks if limit else 1), where
                    want = cuts_of(batch.lens, limit or 1 << 40, paired=paired, use16=i16)
                    assert sw_stats["backtrace_bytes"] == sum(a for _, _, a in want), where
                    assert_same(res, reference["res"])                        # which the composer has checked
                    if limit:
                        assert check_against_composer(sw_oracle, batch.regions, res) == reference["counters"][2]
                        fused = realign.regions_to_ref(batch.regions, batch.mapqs, batch.to_ref, ref_stride=16)
                        assert_same(fused, reference["fused"], to_ref=True)
                monkeypatch.setenv("MGX_SW_ARENA_LIMIT", str(MIB))           # the long haplotype's call is a chunked one
                res = long_realign.regions_to_ref(with_long.regions, with_long.mapqs, with_long.to_ref, ref_stride=16)
                sw_stats = long_sw.stats()
                assert sw_stats["n_pairs_strip"] == 1 and sw_stats["n_pairs"] == len(with_long.lens) and (sw_stats["n_pairs_i16"] > 0) == bool(i16)
                assert sw_stats["backtrace_bytes"] == sum(a for _, _, a in cuts_of(with_long.lens, MIB, paired=paired, use16=i16))
                check_plan(plans, res, long_realign)
                assert_same(res[:1] + res[2:], reference["res"])
                if first_long is None:
                    first_long = res
                    check_against_composer(sw_oracle, with_long.regions, res)
                    check_to_ref_of_regions(with_long.regions, with_long.to_ref, res, 16)
                assert_same(res, first_long, to_ref=True)
    finally:
        long_sw.close()


# ---- 4. strategies and parameters -------------------------------------------------------------------------------------------------
PARAM_SETS = (RC.TO_BEST_HAPLOTYPE, F.STANDARD_NGS, F.ORIGINAL_DEFAULT)          # match 10, 25, 3
assert F.ORIGINAL_DEFAULT in F.REAL_SETS and len({p[0] for p in PARAM_SETS}) == 3
ALL_STRATEGIES = (RC.SOFTCLIP, RC.INDEL, RC.LEADING_INDEL, RC.IGNORE)


@pytest.fixture(scope="module")
def overhang_batch(sw_oracle):
    return make_overhang_batch(sw_oracle)


def make_overhang_batch(sw_oracle):
    """Three regions (3, 1, 4 haplotypes) whose reads make the strategies disagree: reads that start with 3 bases in front of their
    haplotype's first base, reads that end 3 bases behind its last, both, reads that start inside with a deletion close to their
    start, and the usual mix.  The 3 overhanging bases have quality 10 and insertion quality 10: the PairHMM takes them as an
    insertion for about -3.  On the oracle alone, before any device call: every two strategies differ on some read, per parameter set."""
    rng = np.random.RandomState(53)
    plans = []
    for g, hap_lens in enumerate(((100, 140, 90), (120,), (64, 200, 150, 110))):
        p = Plan(rng, hap_lens)
        for h, L in enumerate(hap_lens):
            hap, R = p.haps[h], min(L - 4, 90)
            front, back = other(hap[0]) + seq(rng, 2), seq(rng, 2) + other(hap[-1])
            p.add("front overhang", h, front + hap[:R], low=(3, 0))
            p.add("back overhang", h, hap[L - R:] + back, low=(0, 3))
            if L + 3 <= 150:                                                  # 2 bases in front, 1 behind: about -4 for the two
                p.add("both overhangs", h, front[:2] + hap + back[2:], low=(2, 1))
            p.add("leading deletion", h, hap[4:7] + hap[9:R])                 # starts inside, two bases missing after three
            p.add("verbatim", h, hap[3:3 + R])                                # a leading (and trailing) deletion under INDEL
            p.cut("sub", h, 60 + 5 * h if L > 80 else 60); p.cut("ins", h, min(70, L - 2)); p.cut("verbatim", h, 20 + 7 * g)
        longest = int(np.argmax(hap_lens))
        p.cut("dropped", longest, 80); p.cut("dropped", longest, 85)
        plans.append(p)
    b = Batch(plans, rng)
    b.oracle = {}
    for params in PARAM_SETS:
        for s in ALL_STRATEGIES:
            b.oracle[params, s] = [sw_oracle.align(np.frombuffer(hap, np.uint8), np.frombuffer(read, np.uint8), params, s)[:2]
                                   for p in plans for hap, read in p.pairs(RC.INDEL)]          # of every kept read
        for i, s in enumerate(ALL_STRATEGIES):
            for t in ALL_STRATEGIES[i + 1:]:
                assert b.oracle[params, s] != b.oracle[params, t], (params, s, t)
    return b


@pytest.mark.parametrize("strategy", ALL_STRATEGIES, ids=("SOFTCLIP", "INDEL", "LEADING_INDEL", "IGNORE"))
def test_every_strategy_and_three_parameter_sets(realign, sw_oracle, overhang_batch, strategy):
    """Gaps "overhang strategies" (LEADING_INDEL has not reached the fused call) and "score parameters" (a verbatim read's score is
    len * match on the host, scatter_reads; only TO_BEST_HAPLOTYPE has been passed).  Reached: the oracle's answers differ between
    every two strategies on these reads (overhang_batch), the three sets have three values of match."""
    b = overhang_batch
    n_verbatim = sum(p.n_verbatim(strategy) for p in b.plans)
    assert (n_verbatim > 0) == (strategy in SHORTCUT)
    for params in PARAM_SETS:
        res = realign.regions(b.regions, b.mapqs, strategy=strategy, params=params)
        st = check_plan(b.plans, res, realign, strategy)
        assert st["n_verbatim"] == n_verbatim and realign.sw.stats()["n_pairs"] == st["n_sw_pairs"]
        assert check_against_composer(sw_oracle, b.regions, res, strategy, params) == n_verbatim
        n_scores = 0
        for p, o in zip(b.plans, res):
            for r, (bases, kind, _, _) in enumerate(p.reads):
                if kind == "verbatim" and strategy in SHORTCUT:
                    assert (o["score"][r], o["cigar"][r]) == (len(bases) * params[0], b"%dM" % len(bases)), (params, r)
                    n_scores += 1
        assert n_scores == n_verbatim
        # the kept reads that went through the aligner hold what the oracle gave above
        got = [(o["cigar"][r], int(o["offset"][r])) for p, o in zip(b.plans, res) for r, (_, kind, _, _) in enumerate(p.reads) if kind != "dropped"]
        want = b.oracle[params, strategy]
        skip = [kind == "verbatim" and strategy in SHORTCUT for p in b.plans for _, kind, _, _ in p.reads if kind != "dropped"]
        assert [g for g, s in zip(got, skip) if not s] == [w for w, s in zip(want, skip) if not s]
    if strategy == RC.LEADING_INDEL:
        params = F.ORIGINAL_DEFAULT
        fused = realign.regions_to_ref(b.regions, b.mapqs, b.to_ref, strategy=strategy, params=params, ref_stride=16)
        check_plan(b.plans, fused, realign, strategy)
        assert_same(fused, res)                                               # the last parameter set of the loop is this one
        seen = check_to_ref_of_regions(b.regions, b.to_ref, fused, 16)
        assert realign.to_ref_stats()["n_status"] == [seen.get(s, 0) for s in range(6)] and seen[C.DROPPED] == 6 and seen.get(C.OK, 0) > 0, seen


# ---- 5. one chunk of at least 16 384 pairs ----------------------------------------------------------------------------------------
def slice_reads(d, mapq, t, lo, hi):
    """reads [lo, hi) of a region as a region of its own, with its MAPQs and its to-reference part"""
    ro = d["read_off"].astype(np.int64)
    out = dict(d)
    for k in ("bases", "qual", "ins", "dele", "gcp"):
        out[k] = d[k][ro[lo]:ro[hi]].copy()
    out["read_off"] = (ro[lo:hi + 1] - ro[lo]).astype(np.uint64)
    return out, mapq[lo:hi].copy(), dict(t, hard_clips=None if t["hard_clips"] is None else t["hard_clips"][lo:hi].copy())


def joined(first, second, to_ref):
    out = []
    for a, b in zip(first, second):
        o = {k: np.concatenate([a[k], b[k]]) for k in ("log10", "keep", "best", "offset", "score") + (("start", "status", "n_ref_cigar") if to_ref else ())}
        o["cigar"] = a["cigar"] + b["cigar"]
        if to_ref:
            o["ref_cigar"] = a["ref_cigar"] + b["ref_cigar"]
        out.append(o)
    return out


def make_big_batch(n_aligned):
    rng = np.random.RandomState(59)
    plans = []
    for g in range(3):
        p = Plan(rng, (64, 64))
        kinds = ["sub"] * (n_aligned // 3 + (g < n_aligned % 3)) + ["verbatim"] * 100 + ["dropped"] * 50
        for r in rng.permutation(len(kinds)):
            p.cut(kinds[r], int(rng.randint(2)), 40 if kinds[r] == "dropped" else 24, low_at_edit=kinds[r] == "sub")
        plans.append(p)
    return Batch(plans, rng)


def test_one_chunk_of_16391_aligner_pairs(realign, sw_oracle, cuts_of, monkeypatch):
    """Gap "emit_text": from 16 384 pairs in a chunk the text stage runs on four threads, which it has never done with the element
    sink attached (regions_to_ref) and, behind the gather, not without it either; from 8192 pairs the paired family is chosen by
    count.  Three regions of two 64-base haplotypes, 16 391 reads of 24 bases with one substitution (at a base of quality 10, which
    costs 1.1, so the read stays above -4), 300 verbatim reads of 24 bases and 150 reads of 40 bases with MAPQ 0 (-5 - 1.8).  The same
    reads in two calls of half of every region are the serial reference, byte for byte.  A half still holds 8195 pairs or more, which
    is over kPairedFrom: the halves run once with MGX_SW_PAIRED=1, where only the text stage differs from the whole call, and once
    with MGX_SW_PAIRED=0, the serial stage behind one lane group per wavefront."""
    n_aligned = 16391
    b = make_big_batch(n_aligned)
    plans = b.plans
    assert len(b.lens) == n_aligned >= THREADED_FROM and set(b.lens) == {(64, 24)} and n_aligned // 2 >= PAIRED_FROM
    cuts = cuts_of(b.lens, 4 << 30, paired=1)                                 # the default arena; the family by count
    assert [(lo, hi) for lo, hi, _ in cuts] == [(0, n_aligned)]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    res = realign.regions(b.regions, b.mapqs)
    st = check_plan(plans, res, realign)
    sw_stats = realign.sw.stats()
    assert st["n_sw_pairs"] == sw_stats["n_pairs"] == n_aligned and st["n_verbatim"] == 300 and st["n_reads"] - st["n_kept"] == 150
    assert sw_stats["backtrace_bytes"] == cuts[0][2], (sw_stats, cuts)       # laid out as one chunk of the paired family
    assert check_against_composer(sw_oracle, b.regions, res) == 300          # every read
    fused = realign.regions_to_ref(b.regions, b.mapqs, b.to_ref, ref_stride=8)
    n_status = realign.to_ref_stats()["n_status"]
    assert_same(fused, res)
    seen = check_to_ref_of_regions(b.regions, b.to_ref, fused, 8, every=16)
    assert seen.get(C.OK, 0) > 900 and n_status == status_counts(fused) and n_status[C.DROPPED] == 150, (seen, n_status)
    # the serial text stage: two calls of half of every region, in the whole call's family and in the other one
    for paired in ("1", "0"):
        monkeypatch.setenv("MGX_SW_PAIRED", paired)
        halves = []
        for part in (0, 1):
            cut = [slice_reads(d, m, t, *((0, len(m) // 2) if part == 0 else (len(m) // 2, len(m)))) for d, m, t in zip(b.regions, b.mapqs, b.to_ref)]
            regions, mapqs, to_ref = [list(x) for x in zip(*cut)]
            plain = realign.regions(regions, mapqs)
            assert PAIRED_FROM <= realign.stats()["n_sw_pairs"] < THREADED_FROM
            half = realign.regions_to_ref(regions, mapqs, to_ref, ref_stride=8)
            assert_same(half, plain)
            halves.append(half)
        assert_same(joined(*halves, to_ref=True), fused, to_ref=True), paired


# ---- 6. layouts -------------------------------------------------------------------------------------------------------------------
def test_a_region_that_is_a_view_into_larger_arrays(realign, sw_oracle, batch):
    """Gap "region layout": read_off[0] and hap_off[0] are not 0 and the bytes in front are not the region's; stage_tables rebases
    the kernels' tables by them.  Between two ordinary regions, every output of both calls against the plain region's."""
    rng = np.random.RandomState(61)
    p = mixed_plan(rng, (90, 250, 170, 64), 18, aligned=(60, 64))
    d, mapq = p.region()
    view = _subview(d, mapq, rng)
    assert view["read_off"][0] >= 40 and view["hap_off"][0] >= 40 and len(view["bases"]) > len(d["bases"]) + 40
    assert bytes(view["bases"][:int(view["read_off"][0])]) != bytes(d["bases"][:int(view["read_off"][0])])
    plans = [batch.plans[0], p, batch.plans[2]]
    plain_regions, view_regions = [batch.regions[0], d, batch.regions[2]], [batch.regions[0], view, batch.regions[2]]
    mapqs = [batch.mapqs[0], mapq, batch.mapqs[2]]
    to_ref = to_ref_part(plain_regions, rng, hard=True)
    plain = realign.regions_to_ref(plain_regions, mapqs, to_ref, ref_stride=16)
    plain_counts, plain_status = counters(realign), realign.to_ref_stats()["n_status"]
    got = realign.regions_to_ref(view_regions, mapqs, to_ref, ref_stride=16)
    check_plan(plans, got, realign)
    assert counters(realign) == plain_counts and realign.to_ref_stats()["n_status"] == plain_status
    assert_same(got, plain, to_ref=True)
    assert_same(realign.regions(view_regions, mapqs), got)
    check_against_composer(sw_oracle, plain_regions, got)
    check_against_composer(sw_oracle, view_regions, got)                      # RC.sequences goes by the view's own offsets
    seen = check_to_ref_of_regions(view_regions, to_ref, got, 16)
    assert seen[C.DROPPED] == 4 + 3 + 4 and seen.get(C.OK, 0) > 0


def test_a_region_with_reads_and_no_haplotypes(realign, batch, reference):
    """Gap "region without haplotypes": its reads get the next region's hap_base (or, as the last region, the table's end) and are
    never looked up only because keep is 0 for them.  In the middle and at the end of a call that aligns, and alone (the exit of
    run() without a batch)."""
    rng = np.random.RandomState(67)
    reads = [seq(rng, n) for n in (20, 150, 64, 33, 90)]
    empty, mapq = make_region([], reads), np.array([60, 60, 0, 60, 60], dtype=np.uint8)
    assert len(empty["hap_off"]) == 1 and len(empty["read_off"]) == 6
    empty_to_ref = to_ref_part([empty], rng, hard=True)[0]
    n_batch = sum(len(m) for m in batch.mapqs)

    def check_empty(o, fused):
        assert o["log10"].shape == (5, 0) and list(o["keep"]) == [0] * 5
        assert list(o["offset"]) == [RC.NOT_ALIGNED] * 5 and o["cigar"] == [b""] * 5 and list(o["score"]) == [0] * 5
        if fused:
            assert list(o["status"]) == [C.DROPPED] * 5 and list(o["start"]) == [0] * 5 and list(o["n_ref_cigar"]) == [0] * 5

    for at in (1, 3):                                                         # in the middle, as the last region
        regions, mapqs, to_ref = list(batch.regions), list(batch.mapqs), list(batch.to_ref)
        regions.insert(at, empty); mapqs.insert(at, mapq); to_ref.insert(at, empty_to_ref)
        res = realign.regions(regions, mapqs)
        want = (n_batch + 5,) + reference["counters"][1:]
        assert counters(realign) == want, at
        check_empty(res[at], False)
        assert_same(res[:at] + res[at + 1:], reference["res"])
        fused = realign.regions_to_ref(regions, mapqs, to_ref, ref_stride=16)
        n_status = realign.to_ref_stats()["n_status"]
        assert counters(realign) == want, at
        check_empty(fused[at], True)
        assert_same(fused[:at] + fused[at + 1:], reference["fused"], to_ref=True)
        assert n_status == [n + 5 * (s == C.DROPPED) for s, n in enumerate(reference["n_status"])], at
    # nothing but such regions: no test case, no batch
    fused = realign.regions_to_ref([empty, empty], [mapq, mapq], [empty_to_ref, empty_to_ref], ref_stride=16)
    check_empty(fused[0], True); check_empty(fused[1], True)
    assert counters(realign) == (10, 0, 0, 0) and realign.to_ref_stats()["n_status"] == [0, 10, 0, 0, 0, 0]
    res = realign.regions([empty], [mapq])
    check_empty(res[0], False)
    assert counters(realign) == (5, 0, 0, 0)


def make_plans_of_shared_haplotypes():
    rng = np.random.RandomState(71)
    plans = []
    hap0 = seq(rng, 200)
    haps = [hap0, seq(rng, 9) + hap0[:150] + seq(rng, 60), seq(rng, 180)]
    shared = Plan(rng, (150,))
    shared.haps = [hap0[:150]]
    for r in range(12):
        shared.cut(("sub", "verbatim", "ins", "dropped")[r % 4], 0, 100)      # the same reads in both regions, out of the shared bases
    for g in range(2):
        p = Plan(rng, ())
        p.haps = list(haps)
        for bases, kind, _, _ in shared.reads:
            p.add(kind, 1 - g, bases)                                         # best on 1 - g, by priority
            if kind in ("verbatim", "dropped"):
                assert RC.last_index_of(haps[1], bases) == RC.last_index_of(haps[0], bases) + 9
        plans.append(p)
    p = Plan(rng, ())                                                         # the same three haplotypes with the first two exchanged
    p.haps = [haps[1], haps[0], haps[2]]
    for bases, kind, _, _ in shared.reads:
        p.add(kind, 0, bases)
    plans.append(p)
    return plans, haps


def test_two_regions_of_the_same_haplotypes_under_different_priorities(realign, sw_oracle, batch):
    """Gap "region layout", hap_base: two regions hold the same haplotype bytes; haplotype 1 is haplotype 0's first 150 bases behind
    9 others, so a read out of those 150 bases is 0.04 apart in log10 on the two (the lengths, 200 and 219) and the priorities
    decide: 1 in the first region, 0 in the second.  The read then lies 9 bases further right in the first region than in the second.
    Two regions of the same bytes cannot tell a hap_base that confuses just the two of them, so a third holds the same haplotypes
    with the first two exchanged and the priority on its index 0: a hap_base into either of the others puts its reads 9 bases left."""
    plans, haps = make_plans_of_shared_haplotypes()
    made = [p.region() for p in plans]
    regions, mapqs = [batch.regions[0]] + [d for d, _ in made], [batch.mapqs[0]] + [m for _, m in made]
    assert bytes(regions[1]["hap_bases"]) == bytes(regions[2]["hap_bases"]) != bytes(regions[3]["hap_bases"])
    pri = [None, np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])]
    res = realign.regions(regions, mapqs, priorities=pri)
    check_plan([batch.plans[0]] + plans, res, realign)
    differ = 0
    for o, p in zip(res, pri):
        assert list(o["best"]) == [RC.search_best_allele(row, p) for row in o["log10"]]
        differ += sum(RC.search_best_allele(row, p) != RC.search_best_allele(row, None) for row in o["log10"]) if p is not None else 0
    assert differ >= 18                                                       # the kept reads of the first and the third of the regions
    check_against_composer(sw_oracle, regions, res)
    n_checked = 0
    for r, (bases, kind, _, _) in enumerate(plans[0].reads):
        if kind == "verbatim":
            at = RC.last_index_of(haps[0], bases)
            assert (res[1]["offset"][r], res[2]["offset"][r], res[3]["offset"][r]) == (at + 9, at, at + 9), r
            n_checked += 1
    assert n_checked == 3
    aligned = [r for r, (_, kind, _, _) in enumerate(plans[0].reads) if kind in ("sub", "ins")]
    assert len(aligned) == 6 and all(res[1]["offset"][r] == res[2]["offset"][r] + 9 == res[3]["offset"][r] for r in aligned)
