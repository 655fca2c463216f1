"""mgx_read_to_ref and mgx_realign_regions_to_ref (include/mgx_realign.h) on the device: the read -> reference CIGAR and start against
the reference's own answers (tests/golden/read_to_ref.npz) and against the sequential restatement (read_to_ref_cases.py) at the
kernel's seams, the fused call against mgx_realign_regions on the same input and the restatement on that call's own results, and
the existing calls before and after."""
import ctypes
import os

import numpy as np
import pytest

import read_to_ref_cases as C
import realign_cases as RC
from test_realign_gpu import cut_reads_out_of_haplotypes, gather_region, make_region

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def realign(pkg, engine, sw_engine):
    return pkg.RealignEngine(engine, sw_engine)


@pytest.fixture(scope="module")
def shape_cases():
    return C.shape_cases()


def run_cases(realign, cl, stride):
    """every case a read with a haplotype and a reference haplotype of its own"""
    n = len(cl)
    return realign.to_ref([c["read"] for c in cl], [c["offset"] for c in cl], [C.encode(c["sw"]) for c in cl], np.arange(n),
                          [C.encode(c["hap"]) for c in cl], [c["hap_start"] for c in cl], np.arange(n), [c["ref"] for c in cl],
                          [c["reference_start"] for c in cl], hard_clips=[c["hard"] for c in cl], stride=stride)


def check_cases(realign, cl):
    """the device against the restatement, case sets grouped by their row capacity; returns the statuses seen"""
    seen = set()
    for stride in sorted({c["stride"] for c in cl}):
        use = [c for c in cl if c["stride"] == stride]
        status, start, cigars, n_cigar = run_cases(realign, use, stride)
        for r, c in enumerate(use):
            w_status, w_start, w_el = C.to_ref(c)
            where = (c["name"], C.text_of(c["sw"]), c["offset"], C.text_of(c["hap"]), c["hard"], stride)
            assert status[r] == w_status, where + (int(status[r]), w_status)
            seen.add(w_status)
            if w_status == C.OK:
                assert start[r] == w_start and list(cigars[r]) == list(w_el), where + (int(start[r]), w_start, C.text_of(C.decode(cigars[r])), C.text_of(C.decode(w_el)))
            else:
                assert start[r] == 0 and n_cigar[r] == (len(w_el) if w_status == C.NO_ROOM else 0), where
    return seen


def test_the_seams_against_the_reference_and_the_restatement(realign, shape_cases):
    names = " ".join(c["name"] for c in shape_cases)
    for must in ("indel1_", "indel2_", "indel63_", "indel64_", "indel65_", "_p1", "_p2", "_p3", "_p7", "ref1D", "ref63", "ref64", "ref65", "ref129",
                 "ref1025", "one_base_ref1 ", "hap_is_ref1025", "homoD1025", "homoI1025"):
        assert must in names + " ", must
    seen = check_cases(realign, shape_cases)
    assert seen == {C.OK, C.UNCHANGED, C.THROWS, C.UNDEFINED, C.NO_ROOM}
    # the reference's own answers: the list before the hard clips go around it, in rows of ample capacity
    z = np.load(os.path.join(ROOT, "tests", "golden", "read_to_ref.npz"))
    assert int(z["shape_digest"][0]) == C.digest(shape_cases)
    use = [dict(shape_cases[int(i)], hard=(0, 0)) for i in z["shape_index"]]
    status, start, cigars, _ = run_cases(realign, use, 24)
    off = z["shape_off"]
    moved = 0
    for j, c in enumerate(use):
        assert status[j] == z["shape_status"][j], c["name"]
        if status[j] == C.OK:
            assert start[j] == z["shape_start"][j] and list(cigars[j]) == list(z["shape_elements"][off[j]:off[j + 1]]), c["name"]
            moved += bool(C.categories(c)[1] & {"moved_left", "moved_to_start"})
    assert moved >= 40, moved                                                 # the left-alignment did something in many of them


def test_the_cpu_test_cases_on_the_device(realign):
    cl = C.cases()
    seen = check_cases(realign, cl)
    assert seen == {C.OK, C.UNCHANGED, C.THROWS, C.UNDEFINED, C.NO_ROOM}
    st = realign.to_ref_stats()                                               # of the last call: one capacity group
    assert sum(st["n_status"]) == sum(c["stride"] == max(x["stride"] for x in cl) for c in cl) and st["n_status"][C.DROPPED] == 0


def test_one_read_five_reads_and_the_row_capacity(realign):
    hand = [dict(c, read=c["read"][:10]) if i == 1 else c for i, (c, _, _) in enumerate(C.HAND)]
    for use in (hand[:1], hand[:5], []):                                      # one wavefront; a second workgroup with one; no read
        status, start, cigars, _ = run_cases(realign, use, 8)
        assert len(status) == len(use)
        for r, c in enumerate(use):
            _, text, want_start = C.HAND[r]
            assert (status[r], start[r], C.text_of(C.decode(cigars[r]))) == (C.OK, want_start, text), r
    c = dict(hand[1], hard=(3, 4))                                            # 3H 4M2I2M3D2M 4H: 7 elements
    status, start, cigars, n_cigar = run_cases(realign, [c], 7)
    assert status[0] == C.OK and C.text_of(C.decode(cigars[0])) == "3H4M2I2M3D2M4H" and start[0] == 2
    status, start, cigars, n_cigar = run_cases(realign, [c, hand[0]], 6)
    assert list(status) == [C.NO_ROOM, C.OK] and n_cigar[0] == 7 and C.text_of(C.decode(cigars[1])) == "2I6M2I"
    status, _, _, n_cigar = run_cases(realign, [c], 1)
    assert status[0] == C.NO_ROOM and n_cigar[0] == 7


def test_argument_errors_return_before_any_launch(realign, pkg):
    good = dict(C.HAND[0][0])
    run_cases(realign, [good], 8)
    before = realign.to_ref_stats()
    assert before["n_status"][C.OK] == 1
    for what, kwargs in (("operator code 9 in the aligner's list", dict(sw_cigars=[np.array([3 << 4 | 9], np.uint32)])),
                         ("operator code 15 in the haplotype's list", dict(hap_cigars=[np.array([20 << 4 | 15], np.uint32)])),
                         ("haplotype index out of range", dict(read_hap=[1])),
                         ("reference index out of range", dict(read_ref=[7]))):
        args = dict(reads=[good["read"]], sw_offset=[3], sw_cigars=[C.encode(good["sw"])], read_hap=[0], hap_cigars=[C.encode(good["hap"])],
                    hap_start=[5], read_ref=[0], refs=[good["ref"]], reference_start=[0])
        args.update(kwargs)
        with pytest.raises(pkg.MgxError, match="libmgx error -22"):
            realign.to_ref(**args)
        assert realign.to_ref_stats() == before, what                         # the call did not get as far as resetting them
    inp = pkg.native.ToRefInput(n_reads=1)                                    # every array NULL
    one = np.zeros(4, np.uint32)
    rc = realign.lib.mgx_read_to_ref(realign.pairhmm.ctx, ctypes.byref(inp), one.ctypes.data, one.ctypes.data, 4, one.ctypes.data, one.ctypes.data)
    assert rc == -22 and realign.to_ref_stats() == before


# ---- the fused call ---------------------------------------------------------------------------------------------------------------
def hap_cigars_for(d, rng):
    """a haplotype -> reference CIGAR per haplotype whose read length is the haplotype's: the first is the reference haplotype (nM),
    the others hold an insertion, a deletion or both"""
    lens = np.diff(d["hap_off"].astype(np.int64))
    out = []
    for h, L in enumerate(lens):
        L = int(L)
        kind = 0 if h == 0 else 1 + h % 3
        a = int(rng.randint(1, max(L // 2, 2)))
        i, dl = int(rng.randint(1, 6)), int(rng.randint(1, 6))
        if kind == 0 or L < 20:
            cig = [(L, "M")]
        elif kind == 1:
            cig = [(a, "M"), (i, "I"), (L - a - i, "M")]
        elif kind == 2:
            cig = [(a, "M"), (dl, "D"), (L - a, "M")]
        else:
            cig = [(a, "M"), (dl, "D"), (3, "M"), (i, "I"), (L - a - 3 - i, "M")]
        assert C.read_length(cig) == L
        out.append(C.encode(cig))
    return out


def to_ref_part(regions, rng, hard=False):
    out = []
    for g, d in enumerate(regions):
        nr, nh = len(d["read_off"]) - 1, len(d["hap_off"]) - 1
        out.append(dict(hap_cigars=hap_cigars_for(d, rng), hap_start=rng.randint(0, 5, nh), ref_hap=0, reference_start=1000 * (g + 1),
                        hard_clips=rng.randint(0, 3, (nr, 2)) * 5 if hard else None))
    return out


def check_to_ref_of_regions(regions, to_ref, res, ref_stride, every=1):
    """start, ref_cigar and status against the restatement applied to the call's own best, offset and cigar; `every`: of each
    region's reads, those whose index is a multiple of it"""
    seen = {}
    for g, (d, t, o) in enumerate(zip(regions, to_ref, res)):
        haps, reads = RC.sequences(d)
        for r, read in enumerate(reads):
            if r % every:
                continue
            if not o["keep"][r]:
                want = (C.DROPPED, 0, [])
            else:
                h = int(o["best"][r])
                hard = (0, 0) if t["hard_clips"] is None else tuple(int(x) for x in t["hard_clips"][r])
                c = C.case(o["cigar"][r].decode(), int(o["offset"][r]), C.decode(t["hap_cigars"][h]), int(t["hap_start"][h]), haps[t["ref_hap"]],
                           read, t["reference_start"], hard, stride=ref_stride)
                status, start, el = C.to_ref(c)
                want = (status, start if status == C.OK else 0, list(el) if status == C.OK else [])
            got = (int(o["status"][r]), int(o["start"][r]), list(o["ref_cigar"][r]))
            assert got == want, (g, r, o["cigar"][r], int(o["offset"][r]), got, want)
            seen[want[0]] = seen.get(want[0], 0) + 1
    return seen


def test_the_fused_call_on_a_small_batch(realign, synth):
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
    # ... and one region more with constant qualities of 30, whose reads the filter keeps unless their mapq says otherwise
    regions.append(make_region(*RC.sequences(cut_reads_out_of_haplotypes(
        synth.gen_pairhmm_region(48, 9, 0xA11CE + 9, r_range=(20, 151), h_range=(64, 300)), rng))))
    mapqs = [np.full(len(d["read_off"]) - 1, 60, dtype=np.uint8) for d in regions]
    mapqs[0][::7] = 0                                                         # some reads the filter drops
    mapqs[4][::5] = 0
    pri = [rng.randint(0, 3, len(d["hap_off"]) - 1).astype(np.float64) for d in regions]
    to_ref = to_ref_part(regions, rng, hard=True)
    plain = realign.regions(regions, mapqs, priorities=pri)
    plain_stats = realign.stats()
    res = realign.regions_to_ref(regions, mapqs, to_ref, priorities=pri, ref_stride=12)
    stats = realign.stats()
    for o, p in zip(res, plain):                                              # its regions() part, byte for byte
        for k in ("log10", "keep", "best", "offset", "score"):
            assert np.array_equal(o[k], p[k]), k
        assert o["cigar"] == p["cigar"]
    for k in ("n_reads", "n_kept", "n_verbatim", "n_sw_pairs"):
        assert stats[k] == plain_stats[k], k
    seen = check_to_ref_of_regions(regions, to_ref, res, 12)
    print("fused call: reads per status", seen, "verbatim", stats["n_verbatim"], "aligned", stats["n_sw_pairs"])
    assert seen.get(C.DROPPED, 0) > 0 and seen.get(C.OK, 0) > 0, seen
    assert stats["n_verbatim"] > 0 and stats["n_sw_pairs"] > 0               # both kinds of kept reads went through the kernel
    st = realign.to_ref_stats()
    assert st["n_status"] == [seen.get(s, 0) for s in range(6)], (st, seen)
    indels = sum(any((int(e) & 15) in (1, 2) for e in c) for o in res for c in o["ref_cigar"])
    assert indels > 0, indels                                                 # the haplotypes' insertions and deletions came through
    # a call without regions
    assert realign.regions_to_ref([], [], []) == [] and realign.to_ref_stats()["n_status"] == [0] * 6


@pytest.mark.parametrize("name, dropped, verbatim_all, strategy", [
    ("first and last read dropped", (0, 6), False, RC.SOFTCLIP),
    ("every read dropped", tuple(range(7)), False, RC.SOFTCLIP),
    ("every read verbatim", (), True, RC.SOFTCLIP),
    ("INDEL: the shortcut does not apply", (3,), False, RC.INDEL),
])
def test_the_fused_call_with_and_without_the_verbatim_shortcut(realign, name, dropped, verbatim_all, strategy):
    rng = np.random.RandomState(17)
    d, mapq = gather_region(rng, dropped, verbatim_all)
    to_ref = to_ref_part([d], rng)
    to_ref[0]["hap_cigars"][0] = C.encode([(100, "M"), (4, "D"), (60, "M"), (3, "I"), (97, "M")])      # the best haplotype of every read: 260 bases
    to_ref[0]["ref_hap"] = 1
    res = realign.regions_to_ref([d], [mapq], to_ref, strategy=strategy)
    plain = realign.regions([d], [mapq], strategy=strategy)
    assert res[0]["cigar"] == plain[0]["cigar"] and np.array_equal(res[0]["offset"], plain[0]["offset"])
    assert [r for r in range(7) if res[0]["status"][r] == C.DROPPED] == list(dropped), name
    seen = check_to_ref_of_regions([d], to_ref, res, 16)
    st = realign.stats()
    if strategy == RC.INDEL:
        assert st["n_verbatim"] == 0 and st["n_sw_pairs"] == 6
    elif verbatim_all:
        assert st["n_verbatim"] == 7 and seen == {C.OK: 7}
    assert realign.to_ref_stats()["n_status"] == [seen.get(s, 0) for s in range(6)]


def test_existing_calls_are_unchanged_by_a_to_reference_call(realign, engine, sw_engine, synth):
    rng = np.random.RandomState(29)
    d = cut_reads_out_of_haplotypes(synth.gen_pairhmm_region(30, 6, 77, r_range=(20, 151), h_range=(64, 300)), rng)
    mapq = np.full(30, 60, dtype=np.uint8)
    w = synth.gen_sw_pairs(200, 9, ref_range=(30, 300), alt_range=(10, 150))
    align = lambda: sw_engine.align_batch(w["ref_off"], w["ref"], w["alt_off"], w["alt"], w["strategy"], want_score=True)  # noqa: E731

    def existing():
        sw, sw_stats = align(), sw_engine.stats()
        re, re_stats = realign.regions([d], [mapq]), realign.stats()
        return sw, sw_stats, re, re_stats, engine.regions([d], [mapq])
    before = existing()
    realign.regions_to_ref([d], [mapq], to_ref_part([d], rng))
    run_cases(realign, [C.HAND[0][0]], 8)
    after = existing()
    assert before[0][0] == after[0][0] and np.array_equal(before[0][1], after[0][1]) and np.array_equal(before[0][2], after[0][2])
    for k in ("n_pairs", "cells", "n_launches", "backtrace_bytes", "n_pairs_i16", "n_pairs_strip", "n_strips"):
        assert before[1][k] == after[1][k], k
    for k in ("log10", "keep", "best", "offset", "score"):
        assert np.array_equal(before[2][0][k], after[2][0][k]), k
    assert before[2][0]["cigar"] == after[2][0]["cigar"]
    for k in ("n_reads", "n_kept", "n_verbatim", "n_sw_pairs"):
        assert before[3][k] == after[3][k], k
    assert np.array_equal(before[4][0][0], after[4][0][0]) and np.array_equal(before[4][0][1], after[4][0][1])
