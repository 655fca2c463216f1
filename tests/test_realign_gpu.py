"""mgx_realign_regions and mgx_pairhmm_best_alleles (include/mgx_realign.h) on the device: the likelihoods against PairHMMEngine.regions,
the best haplotype against the sequential restatement of searchBestAllele on those very doubles, the alignments against
SmithWatermanEngine.align_batch on host-assembled pairs and against the composer over the CPU oracle (realign_cases.py), and the
seams of the verbatim search and of the gather."""
import numpy as np
import pytest

import realign_cases as RC

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def seq(rng, n):
    return ACGT[rng.randint(0, 4, n)].tobytes()


def other(base):
    """another base than this one, as bytes"""
    return bytes([{65: 67, 67: 71, 71: 84, 84: 65}.get(base, 65)])


def make_region(haps, reads, qual=30):
    """a region dict in the cross-product form from lists of bytes, constant qualities"""
    def pack(xs):
        off = np.zeros(len(xs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in xs], dtype=np.uint64)
        return off, np.frombuffer(b"".join(xs), dtype=np.uint8).copy()
    read_off, bases = pack(reads)
    hap_off, hap_bases = pack(haps)
    n = len(bases)
    return dict(read_off=read_off, bases=bases, qual=np.full(n, qual, dtype=np.uint8), ins=np.full(n, 45, dtype=np.uint8),
                dele=np.full(n, 45, dtype=np.uint8), gcp=np.full(n, 10, dtype=np.uint8), hap_off=hap_off, hap_bases=hap_bases)


def cut_reads_out_of_haplotypes(d, rng):
    """replaces the reads' bases of a synth.gen_pairhmm_region dict by pieces of its haplotypes: about half verbatim, the others with a
    substitution, a deletion or an insertion; a read longer than its haplotype is the haplotype plus a random tail.  Lengths stay."""
    haps, reads = RC.sequences(d)
    bases = np.array(d["bases"], dtype=np.uint8)
    ro = d["read_off"].astype(np.int64)
    for r, read in enumerate(reads):
        R = len(read)
        hap = haps[rng.randint(len(haps))]
        if len(hap) < R + 1:
            new = hap + seq(rng, R - len(hap))
        else:
            at = rng.randint(0, len(hap) - R)
            kind = rng.randint(0, 6)
            p = rng.randint(0, R)
            if kind < 3 or R < 4:
                new = hap[at:at + R]
            elif kind == 3:
                new = hap[at:at + p] + other(hap[at + p]) + hap[at + p + 1:at + R]
            elif kind == 4:
                new = hap[at:at + p] + hap[at + p + 1:at + R + 1]
            else:
                new = hap[at:at + p] + seq(rng, 1) + hap[at + p:at + R - 1]
        assert len(new) == R
        bases[ro[r]:ro[r + 1]] = np.frombuffer(new, dtype=np.uint8)
    d = dict(d)
    d["bases"] = bases
    return d


@pytest.fixture(scope="module")
def realign(pkg, engine, sw_engine):
    return pkg.RealignEngine(engine, sw_engine)


def host_pairs(regions, results, strategy):
    """the aligner's input as a caller assembles it on the host today: kept reads that rfind does not find, against their best haplotype"""
    refs, alts, where = [], [], []
    for g, (d, o) in enumerate(zip(regions, results)):
        haps, reads = RC.sequences(d)
        for r, read in enumerate(reads):
            hap = haps[int(o["best"][r])] if o["keep"][r] else b""
            if o["keep"][r] and (strategy not in (RC.SOFTCLIP, RC.IGNORE) or RC.last_index_of(hap, read) < 0):
                refs.append(hap); alts.append(read); where.append((g, r))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
    cat = lambda xs: np.frombuffer(b"".join(xs), dtype=np.uint8)  # noqa: E731
    return dict(ref_off=off(refs), ref=cat(refs), alt_off=off(alts), alt=cat(alts), strategy=np.full(len(refs), strategy, dtype=np.uint8)), where


def check_against_composer(sw_oracle, regions, results, strategy=RC.SOFTCLIP, params=RC.TO_BEST_HAPLOTYPE):
    n_verbatim = 0
    for g, (d, o) in enumerate(zip(regions, results)):
        haps, reads = RC.sequences(d)
        cig, off, sc, nv = RC.compose(sw_oracle, haps, reads, o["best"], o["keep"], strategy, params)
        assert o["cigar"] == cig, (g, [(a, b) for a, b in zip(o["cigar"], cig) if a != b][:3])
        assert np.array_equal(o["offset"], off) and np.array_equal(o["score"], sc), g
        n_verbatim += nv
    return n_verbatim


def check_stats(realign, results, n_verbatim):
    st = realign.stats()
    n_reads = sum(len(o["keep"]) for o in results)
    n_kept = sum(int(o["keep"].sum()) for o in results)
    assert (st["n_reads"], st["n_kept"], st["n_verbatim"], st["n_sw_pairs"]) == (n_reads, n_kept, n_verbatim, n_kept - n_verbatim), st
    return st


def test_best_alleles_on_the_rows_of_the_host_test(realign):
    rows = RC.rule_rows()
    for with_pri in (True, False):
        use = [(n, v, p) for n, v, p in rows if (p is not None) == with_pri]
        got = realign.best_alleles([v for _, v, _ in use], [p for _, _, p in use] if with_pri else None)
        want = [RC.search_best_allele(v, p) for _, v, p in use]
        bad = [(n, int(g), w) for (n, _, _), g, w in zip(use, got, want) if g != w]
        assert not bad, bad[:5]
    assert len(realign.best_alleles([])) == 0


def test_the_whole_call_on_a_small_batch(realign, engine, sw_engine, sw_oracle, synth):
    rng = np.random.RandomState(11)
    regions = []
    for k, (nr, nh) in enumerate(((60, 17), (5, 1), (0, 3), (40, 65))):
        d = synth.gen_pairhmm_region(max(nr, 1), nh, 0xA11CE + k, r_range=(20, 151), h_range=(64, 300))
        if nr == 0:
            haps, _ = RC.sequences(d)
            d = make_region(haps, [])
        else:
            d = cut_reads_out_of_haplotypes(d, rng)
        regions.append(d)
    mapqs = [np.full(len(d["read_off"]) - 1, 60, dtype=np.uint8) for d in regions]
    pri = [rng.randint(0, 3, len(d["hap_off"]) - 1).astype(np.float64) for d in regions]
    res = realign.regions(regions, mapqs, priorities=pri)
    plain = engine.regions(regions, mapqs)
    changed = 0
    for o, (log10, keep), p in zip(res, plain, pri):
        assert np.array_equal(o["log10"], log10) and np.array_equal(o["keep"], keep)
        want = [RC.search_best_allele(row, p) for row in o["log10"]]          # on the device's own doubles: 1e-5 may flip a tie
        assert list(o["best"]) == want
        changed += sum(w != RC.search_best_allele(row, None) for w, row in zip(want, o["log10"]))
    assert changed > 0                                                        # the priorities decided somewhere
    # the aligner on host-assembled pairs: byte-identical
    w, where = host_pairs(regions, res, RC.SOFTCLIP)
    stride = 2 * max(int(np.diff(d[k].astype(np.int64)).max(initial=1)) for d in regions for k in ("read_off", "hap_off")) + 1
    cig, off, sc = sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], params=RC.TO_BEST_HAPLOTYPE, stride=stride,
                                         want_score=True)
    for (g, r), c, o_, s in zip(where, cig, off, sc):
        assert (res[g]["cigar"][r], res[g]["offset"][r], res[g]["score"][r]) == (c, o_, s), (g, r)
    n_verbatim = check_against_composer(sw_oracle, regions, res)
    st = check_stats(realign, res, n_verbatim)
    assert st["n_verbatim"] > 0 and st["n_sw_pairs"] > 0 and st["n_sw_pairs"] == len(where)
    # without priorities: the likelihood-best, first index
    res0 = realign.regions(regions, mapqs)
    for o in res0:
        assert list(o["best"]) == [RC.search_best_allele(row, None) for row in o["log10"]]


def unique_at(rng, H, R, at):
    """(haplotype of H bases, read of R) whose only occurrence starts at `at`"""
    while True:
        hap = seq(rng, H)
        read = hap[at:at + R]
        if hap.find(read) == hap.rfind(read) == at:
            return hap, read


def test_seams_of_the_verbatim_search(realign, sw_oracle):
    rng = np.random.RandomState(5)
    cases = {}
    hap = seq(rng, 90)
    cases["read == haplotype"] = (hap, hap, 0)
    hap = seq(rng, 80)
    cases["read one base longer than the haplotype"] = (hap, hap + b"A", -1)
    hap = b"CCCCCCCCCCGCCCCCCCCCCCCCCCCCCC"
    cases["a 1-base read"] = (hap, b"G", 10)
    cases["only occurrence at 0"] = unique_at(rng, 200, 50, 0) + (0,)
    cases["only occurrence at H - R"] = unique_at(rng, 200, 50, 150) + (150,)
    cases["64 start positions, the last one tried matches"] = unique_at(rng, 103, 40, 0) + (0,)
    cases["65 start positions, the second block's only lane matches"] = unique_at(rng, 104, 40, 0) + (0,)
    cases["65 start positions, the first block's last lane matches"] = unique_at(rng, 104, 40, 1) + (1,)
    unit = b"ACGGTCTA"
    hap = seq(rng, 37) + unit * 7 + seq(rng, 41)
    read = unit * 3
    occurrences = [k for k in range(len(hap) - len(read) + 1) if hap[k:k + len(read)] == read]
    assert len(occurrences) == 5
    cases["a tandem repeat with 5 occurrences"] = (hap, read, occurrences[-1])
    hap, read = unique_at(rng, 120, 60, 30)
    hap = hap[:50] + b"A" + hap[51:]
    cases["a lower-case base"] = (hap, hap[30:50] + b"a" + hap[51:90], -1)
    hap = hap[:50] + b"N" + hap[51:]
    cases["a lower-case n against N"] = (hap, hap[30:50] + b"n" + hap[51:90], -1)
    regions = [make_region([h], [r]) for h, r, _ in cases.values()]
    res = realign.regions(regions, [np.array([60], dtype=np.uint8)] * len(regions))
    for (name, (hap, read, at)), o in zip(cases.items(), res):
        assert o["keep"][0] == 1 and o["best"][0] == 0, name                  # the seam is reached
        assert RC.last_index_of(hap, read) == at, name
        if at >= 0:
            assert (o["cigar"][0], o["offset"][0], o["score"][0]) == (b"%dM" % len(read), at, 10 * len(read)), name
    n_verbatim = check_against_composer(sw_oracle, regions, res)
    check_stats(realign, res, n_verbatim)
    assert n_verbatim == sum(at >= 0 for _, _, at in cases.values())


def gather_region(rng, dropped, verbatim_all=False):
    """one haplotype pair, 7 reads of 150 bases cut out of the first haplotype; `dropped`: the reads that get mapq 0 and with it base
    qualities of 6 throughout, which filterPoorlyModeledEvidence drops at this length"""
    haps = [seq(rng, 260), seq(rng, 240)]
    reads = []
    for r in range(7):
        at = rng.randint(0, 100)
        read = haps[0][at:at + 150]
        if not verbatim_all and r % 3 != 1:
            p = 20 + 15 * r
            read = read[:p] + other(read[p]) + read[p + 1:]
        reads.append(read)
    mapq = np.array([0 if r in dropped else 60 for r in range(7)], dtype=np.uint8)
    return make_region(haps, reads), mapq


@pytest.mark.parametrize("name, dropped, verbatim_all, strategy", [
    ("first and last read dropped", (0, 6), False, RC.SOFTCLIP),
    ("every read dropped", tuple(range(7)), False, RC.SOFTCLIP),
    ("every read verbatim", (), True, RC.SOFTCLIP),
    ("IGNORE: the shortcut applies", (3,), False, RC.IGNORE),
    ("INDEL: the shortcut does not apply", (3,), False, RC.INDEL),
])
def test_seams_of_the_gather(realign, sw_oracle, name, dropped, verbatim_all, strategy):
    rng = np.random.RandomState(17)
    d, mapq = gather_region(rng, dropped, verbatim_all)
    res = realign.regions([d], [mapq], strategy=strategy)
    assert [r for r in range(7) if not res[0]["keep"][r]] == list(dropped), name
    for r in dropped:
        assert (res[0]["offset"][r], res[0]["cigar"][r], res[0]["score"][r]) == (RC.NOT_ALIGNED, b"", 0)
    n_verbatim = check_against_composer(sw_oracle, [d], res, strategy)
    st = check_stats(realign, res, n_verbatim)
    if strategy == RC.INDEL:
        assert st["n_verbatim"] == 0 and st["n_sw_pairs"] == 6
    elif verbatim_all:
        assert st["n_sw_pairs"] == 0 and st["n_verbatim"] == 7
    elif len(dropped) == 7:
        assert st["n_kept"] == 0 and st["n_sw_pairs"] == 0
    else:
        assert st["n_verbatim"] > 0 and st["n_sw_pairs"] > 0


def test_a_best_haplotype_of_2049_bases(pkg, engine, sw_engine, sw_oracle):
    rng = np.random.RandomState(23)
    hap = seq(rng, 2049)
    read = hap[1000:1050] + other(hap[1050]) + hap[1051:1120]
    d, mapq = make_region([hap], [read, hap[5:105]]), np.array([60, 60], dtype=np.uint8)
    with pytest.raises(pkg.MgxError, match="libmgx error -7"):                # -E2BIG from the plain context
        pkg.RealignEngine(engine, sw_engine).regions([d], [mapq])
    long_sw = pkg.SmithWatermanEngine(0, pkg.smithwaterman.LONG_REF)
    try:
        long_realign = pkg.RealignEngine(engine, long_sw)
        res = long_realign.regions([d], [mapq])
        assert list(res[0]["keep"]) == [1, 1]
        assert check_against_composer(sw_oracle, [d], res) == 1
        assert long_sw.stats()["n_pairs_strip"] == 1
        check_stats(long_realign, res, 1)
    finally:
        long_sw.close()


def test_contexts_on_different_devices(pkg, engine):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    other = pkg.SmithWatermanEngine(1)
    try:
        d = make_region([b"ACGTACGTACGTACGTACGT"], [b"ACGTACGTAC"])
        with pytest.raises(pkg.MgxError, match="libmgx error -22"):
            pkg.RealignEngine(engine, other).regions([d], [np.array([60], dtype=np.uint8)])
    finally:
        other.close()


def test_existing_calls_are_unchanged_by_a_realign_call(realign, engine, sw_engine, synth):
    rng = np.random.RandomState(29)
    d = cut_reads_out_of_haplotypes(synth.gen_pairhmm_region(30, 6, 77, r_range=(20, 151), h_range=(64, 300)), rng)
    mapq = np.full(30, 60, dtype=np.uint8)
    w = synth.gen_sw_pairs(200, 9, ref_range=(30, 300), alt_range=(10, 150))
    align = lambda: sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)  # noqa: E731
    before_sw, before_hmm = align(), engine.regions([d], [mapq])
    before_stats = sw_engine.stats()
    realign.regions([d], [mapq])
    after_sw, after_hmm = align(), engine.regions([d], [mapq])
    assert before_sw[0] == after_sw[0] and np.array_equal(before_sw[1], after_sw[1]) and np.array_equal(before_sw[2], after_sw[2])
    assert np.array_equal(before_hmm[0][0], after_hmm[0][0]) and np.array_equal(before_hmm[0][1], after_hmm[0][1])
    after_stats = sw_engine.stats()
    for k in ("n_pairs", "cells", "n_launches", "backtrace_bytes", "n_pairs_i16", "n_pairs_strip", "n_strips"):
        assert before_stats[k] == after_stats[k], k                           # the same jobs in the same arena
