"""The PairHMM wire form on the host, without a GPU (csrc/pairhmm_wire.h, mgx_pairhmm_pack_batch_wire and
mgx_pairhmm_wire_expand_host): packing a batch bit by bit and expanding it again gives the canonical form of the packer's
batch -- qualities masked with 127, bases folded to A C T G N -- at every bit phase, for every width, and in the documented
number of bytes."""
import numpy as np
import pytest

import pairhmm_wire_cases as W
from test_queue_cpu import _streams


def round_trip(pkg, d, lo, hi, what=""):
    wire = pkg.pairhmm.pack_batch_wire(d, lo, hi)
    W.assert_same_batch(pkg.pairhmm.wire_expand(wire), W.canonical(pkg.pairhmm.pack_batch(d, lo, hi)), what)
    assert wire["need"] == pkg.pairhmm.wire_need(wire), what
    return wire


@pytest.mark.parametrize("name", ["region", "cross", "independent", "shuffled"])
def test_round_trip_on_the_queue_streams(pkg, synth, name):
    d = _streams(synth)[name]
    n = len(d["pair_read"]) if d.get("pair_read") is not None else (len(d["read_off"]) - 1) * (len(d["hap_off"]) - 1)
    for lo, hi in [(0, 0), (5, 5), (0, 1), (n - 1, n), (3, 4), (0, n), (n // 3, 2 * n // 3), (1, 51), (n - 50, n)]:
        wire = round_trip(pkg, d, lo, hi, (name, lo, hi))
        assert wire["n_pairs"] == hi - lo


def test_reads_start_at_every_bit_phase(pkg):
    """the seven seam lengths in every order: 7-bit qualities, 6-bit gap penalties, a varying gcp"""
    seam = W.seam_stream()
    starts = set()
    for order in W.seam_orders(every=True):
        wire = round_trip(pkg, W.with_order(seam, order), 0, 7, order)
        assert (wire["w_qual"], wire["w_ins"], wire["w_del"], wire["w_gcp"]) == (7, 6, 6, 6)
        starts.update(int(x) % 8 for x in wire["read_off"][:-1])
    # lengths of 0 and +-1 modulo 8, three of +1 and two of -1: reads start two positions before to three after a group's
    # first; the phases 4 and 5 come from the 3- and 5-base reads below
    assert starts == {6, 7, 0, 1, 2, 3}


def test_reads_start_at_the_remaining_phases(pkg):
    for lens in ((3,) * 9, (5,) * 9):
        d = W.stream(lens, (4, 9), seed=41, qmax=127)
        d["gcp"] = np.arange(len(d["gcp"]), dtype=np.uint8)
        wire = round_trip(pkg, d, 0, d["n_pairs"], lens)
        assert (wire["w_qual"], wire["w_gcp"]) == (7, 6) and {int(x) % 8 for x in wire["read_off"][:-1]} == set(range(8))


@pytest.mark.parametrize("name", sorted(W.small_shapes()))
def test_small_shapes(pkg, name):
    d = W.small_shapes()[name]
    round_trip(pkg, d, 0, d["n_pairs"], name)
    round_trip(pkg, d, 0, 1, name)


@pytest.mark.parametrize("case", W.width_cases(), ids=lambda c: c[0])
def test_width_selection(pkg, case):
    name, d, expect = case
    wire = round_trip(pkg, d, 0, d["n_pairs"], name)
    got = {k: wire[k] for k in ("w_qual", "w_ins", "w_del", "w_gcp")}
    assert got == {k: expect[k] for k in got}, name
    if expect["w_gcp"] == 0:
        assert wire["gcp_const"] == expect["gcp_const"] and len(wire["gcp"]) == 0
    groups = (len(d["qual"]) + 7) // 8
    assert [len(wire[k]) for k in ("qual", "ins", "dele", "gcp")] == [groups * got[k] for k in ("w_qual", "w_ins", "w_del", "w_gcp")]


def test_a_byte_of_zero_survives(pkg):
    d = dict(W.stream((5, 16, 20, 9), (12, 7), seed=21))
    for k in ("qual", "ins", "dele", "gcp"):
        d[k] = d[k].copy(); d[k][[0, 7, 8, 33, 49]] = 0
    back = pkg.pairhmm.wire_expand(pkg.pairhmm.pack_batch_wire(d, 0, d["n_pairs"]))
    for k in ("qual", "ins", "dele", "gcp"):
        assert np.array_equal(np.flatnonzero(back[k] == 0), np.flatnonzero(d[k] == 0)), k


def test_bases_fold_to_the_five_letters(pkg):
    for name, d in W.base_cases().items():
        wire = round_trip(pkg, d, 0, d["n_pairs"], name)
        back = pkg.pairhmm.wire_expand(wire)
        assert set(back["bases"]) | set(back["hap_bases"]) <= set(b"ACTGN"), name
    d = W.base_cases()["every_byte"]
    back = pkg.pairhmm.wire_expand(pkg.pairhmm.pack_batch_wire(d, 0, 1))
    for letter in b"ACTGN":
        assert back["bases"][letter] == letter
    others = np.array([b for b in range(256) if b not in b"ACTGN"])
    assert (back["bases"][others] == ord("A")).all()          # lower case, IUPAC, 0x00, 0xFF ... : the kernels' code 0
    assert back["bases"][ord("N")] == ord("N")


def test_sizes(pkg, synth):
    d = W.seam_stream()
    inp, keep = pkg.pairhmm.make_input(d)
    import ctypes as C
    lib = pkg.native.load()
    out = pkg.native.PairHMMWire()
    need = C.c_size_t()
    assert lib.mgx_pairhmm_pack_batch_wire(C.byref(inp), 0, 7, None, 0, C.byref(out), C.byref(need)) == -28
    wire = pkg.pairhmm.pack_batch_wire(d, 0, 7)
    assert need.value == wire["need"] == pkg.pairhmm.wire_need(wire)
    buf = np.zeros(need.value // 8 + 1, dtype=np.uint64)
    assert lib.mgx_pairhmm_pack_batch_wire(C.byref(inp), 0, 7, buf.ctypes.data_as(C.c_void_p), need.value - 1, C.byref(out), C.byref(need)) == -28
    assert need.value == wire["need"]
    assert lib.mgx_pairhmm_pack_batch_wire(C.byref(inp), 0, 7, buf.ctypes.data_as(C.c_void_p), need.value, C.byref(out), C.byref(need)) == 0
    # independent 128 x 256 test cases, qualities up to 63, constant gcp: 64 + 3 * 96 + 128 + 32 bytes per test case cross
    # PCIe instead of 5 * 128 + 256 + 32 = 928; the seven parts of the upload are each rounded up to 256 bytes
    for n in (64, 61):
        s = synth.gen_pairhmm_pairs(n, 7)
        wire = pkg.pairhmm.pack_batch_wire(s, 0, n)
        assert (wire["w_qual"], wire["w_ins"], wire["w_del"], wire["w_gcp"], wire["gcp_const"]) == (6, 6, 6, 0, 10)
        per_case = 64 + 3 * 96 + 128 + 32
        assert per_case == 512
        up, plain = pkg.pairhmm.wire_upload_bytes(wire), pkg.pairhmm.plain_upload_bytes(pkg.pairhmm.pack_batch(s, 0, n))
        pad = up - per_case * n
        assert (pad == 0) if n % 8 == 0 else (0 <= pad < 7 * 256), (n, pad)
        assert 928 * n <= plain < 928 * n + 7 * 256
        assert wire["need"] == 8 * (n + 1) * 2 + 8 * n + (64 + 3 * 96 + 128) * n


def test_pack_wire_rejects_bad_ranges_and_indices(pkg, synth):
    d = synth.gen_pairhmm_pairs(10, 1, r_range=(5, 9), h_range=(5, 9))
    with pytest.raises(pkg.MgxError):
        pkg.pairhmm.pack_batch_wire(d, 5, 11)
    bad = dict(d); bad["pair_read"] = d["pair_read"].copy(); bad["pair_read"][3] = 10
    with pytest.raises(pkg.MgxError, match="test case 3"):
        pkg.pairhmm.pack_batch_wire(bad, 0, 10)
    with pytest.raises(pkg.MgxError, match="test case 3"):          # as pack_batch names it
        pkg.pairhmm.pack_batch(bad, 0, 10)
    pkg.pairhmm.pack_batch_wire(bad, 4, 10)                          # the bad test case is outside the range
