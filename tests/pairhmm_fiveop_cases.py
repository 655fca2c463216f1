"""Shared by the tests of the fp32 PairHMM cell forms and by tools/dev_cell_emulate.py: the one wrapper that builds and
calls the host emulation of the cells (tools/cell_emulator.cpp over csrc/pairhmm_cell.h; form 4: the five-operation cell with its two
deferral rules), the data sets with the one with_qualities, and the static rule restated in numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, _ensure_oracle

CSRC = os.path.join(ROOT, "fast-genomic-data-processing_amd", "csrc")
SO = os.path.join(ROOT, "tools", "bin", "libcell_emulator.so")
SRC = [os.path.join(ROOT, "tools", "cell_emulator.cpp"), os.path.join(CSRC, "mgx_tables.cpp")]
FIVE, STATIC, DYNAMIC, HAP_N, LONG = range(5)        # cell_emulate_paths
TABLES = dict(ph2pr=128, mm=32640, ph2pr_div3=128, gap_ratio=128)      # cell_emulate_tables, in its argument order
# log10 of the float-first threshold as the results are scaled: 1e-28f against INITIAL = 2^120
THRESHOLD = -28.0 - 120.0 * np.log10(2.0)
N = np.uint8(ord("N"))
_LIB = None


def emulator_deps():
    """The emulator's sources and every header of the project they include, directly or not."""
    seen, todo = [], list(SRC)
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen or not os.path.exists(path):
            continue
        seen.append(path)
        with open(path) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                todo += [os.path.join(os.path.dirname(path), inc), os.path.join(CSRC, inc)]
    return seen


def emulator():
    """tools/cell_emulator.cpp as a shared library, built again when a source or a header it includes is newer."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in emulator_deps()):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off",
                                   "-I", CSRC, "-o", SO] + SRC)
        _LIB = C.CDLL(SO)
        for fn in ("cell_emulate_batch", "cell_emulate_paths", "cell_emulate_deferrals", "cell_emulate_tables"):
            getattr(_LIB, fn).restype = None
    return _LIB


def emulate_res(d, form=4):
    """-> (the kernel's fp32 `res` of every test case, the way every test case went: meaningful under form 4).  Without
    pair_read / pair_hap, read k meets haplotype k."""
    lib = emulator()
    n = len(d["pair_read"]) if d.get("pair_read") is not None else len(d["read_off"]) - 1
    pr = np.ascontiguousarray(d["pair_read"] if d.get("pair_read") is not None else np.arange(n), dtype=np.uint32)
    ph = np.ascontiguousarray(d["pair_hap"] if d.get("pair_hap") is not None else np.arange(n), dtype=np.uint32)
    arrs = [np.ascontiguousarray(d[k]) for k in ("read_off", "hap_off", "bases", "qual", "ins", "dele", "gcp", "hap_bases")]
    arrs[0] = arrs[0].astype(np.uint64)
    arrs[1] = arrs[1].astype(np.uint64)
    res = np.empty(n, dtype=np.float32)
    lib.cell_emulate_batch(C.c_int(form), C.c_int(n), C.c_void_p(pr.ctypes.data), C.c_void_p(ph.ctypes.data),
                           *[C.c_void_p(a.ctypes.data) for a in arrs], C.c_void_p(res.ctypes.data))
    way = np.empty(n, dtype=np.uint8)
    lib.cell_emulate_paths(C.c_int(n), C.c_void_p(way.ctypes.data))
    a, b = C.c_uint64(0), C.c_uint64(0)
    lib.cell_emulate_deferrals(C.byref(a), C.byref(b))
    assert (int(a.value), int(b.value)) == (int((way == STATIC).sum()), int((way == DYNAMIC).sum()))
    return res, way


def emulate(d, form=4):
    """-> (log10 values as the kernel scales them, float-first flags, the way every test case went)"""
    res, way = emulate_res(d, form)
    with np.errstate(divide="ignore"):
        log10 = (np.log10(res) - np.float32(np.log10(np.float32(2.0 ** 120)))).astype(np.float64)
    return log10, (~(res >= np.float32(1e-28))).astype(np.uint8), way


def emulator_tables():
    """The four fp32 tables the emulator reads, by name."""
    out = {k: np.empty(n, dtype=np.float32) for k, n in TABLES.items()}
    emulator().cell_emulate_tables(*[C.c_void_p(a.ctypes.data) for a in out.values()])
    return out


def with_qualities(d, seed, qual=(0, 127), ins=(0, 127), dele=(0, 127), gcp=(1, 127), zero_ins_del_rate=0.05):
    """d with every per-base quality drawn again, uniformly from the given ranges; a share of the bases gets
    ins = del = 0, where matchToMatchProb is 0."""
    rng = np.random.RandomState(seed)
    nb = len(d["bases"])
    draw = lambda r: rng.randint(r[0], r[1] + 1, nb).astype(np.uint8)  # noqa: E731
    out = dict(d, qual=draw(qual), ins=draw(ins), dele=draw(dele), gcp=draw(gcp))
    z = rng.rand(nb) < zero_ins_del_rate
    out["ins"][z] = 0
    out["dele"][z] = 0
    return out


def whole_quality_range(synth, n):
    """The "qualities 0-127, gcp (1,127)" set of tools/dev_cell_emulate.py: reads of 1-128 bases."""
    d = synth.gen_pairhmm_pairs(n, 0xC311 + 128, r_range=(1, 128), h_range=(1, 256), hap_n_rate=0.01)
    return with_qualities(d, 7 + 127, gcp=(1, 127))


def has_n(d):
    ho = d["hap_off"].astype(np.int64)
    isn = np.concatenate([[0], np.cumsum(d["hap_bases"] == N)])
    return (isn[ho[1:]] - isn[ho[:-1]])[d["pair_hap"]] > 0


def static_rule(d):
    """Per test case: its read has a row with matchToMatchProb == 0 or a gap-continuation byte of 0 (from the oracle's table)."""
    olib = C.CDLL(_ensure_oracle())
    olib.ph_oracle_init()
    olib.ph_oracle_table_mm_f32.restype = C.POINTER(C.c_float)
    mm = np.ctypeslib.as_array(olib.ph_oracle_table_mm_f32(), (32640,))
    qi, qd = (d["ins"] & 127).astype(np.int64), (d["dele"] & 127).astype(np.int64)
    mn, mx = np.minimum(qi, qd), np.maximum(qi, qd)
    bad = (mm[(mx * (mx + 1)) // 2 + mn] == 0) | ((d["gcp"] & 127) == 0)
    ro = d["read_off"].astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(bad)])
    return (cum[ro[1:]] - cum[ro[:-1]])[d["pair_read"]] > 0


def one_pair(bases, qual, ins, dele, gcp, hap):
    u8 = lambda x: np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)  # noqa: E731
    bases, hap = u8(bases), u8(hap)
    R = len(bases)
    full = lambda v: np.full(R, v, dtype=np.uint8) if np.isscalar(v) else u8(v)  # noqa: E731
    return dict(n_reads=1, n_haps=1, n_pairs=1, read_off=np.array([0, R], dtype=np.uint64), hap_off=np.array([0, len(hap)], dtype=np.uint64),
                bases=bases, qual=full(qual), ins=full(ins), dele=full(dele), gcp=full(gcp), hap_bases=hap,
                pair_read=np.zeros(1, dtype=np.uint32), pair_hap=np.zeros(1, dtype=np.uint32))


def overflowing_pair(R=16):
    """H = 1 and insertion qualities that alternate between 60 and 10: x of the five-operation cell leaves fp32.  The only
    match cell is M[1][1] = INITIAL g e = 1.2e36; X[2][1] = M pMX_2 = 1.2e35 with ins = 10 in row 2, and in row 3 with
    ins = 60 x = X^ / A' = X pXX pMM_3 / pMX_3 = 1.2e34 / 1e-6 > FLT_MAX.  The likelihood itself, X[R][1] = 1.2e35 * 0.1^(R - 2),
    stays far above the float-first threshold."""
    ins = np.where(np.arange(R) % 2 == 0, 60, 10).astype(np.uint8)
    return one_pair(b"ACGT" * (R // 4), 30, ins, 40, 10, b"A")


def cell_bits_cases(synth):
    """The fixed set whose `res` bits tests/golden/pairhmm_cell_bits.npz holds, by name: the whole quality range (N haplotypes,
    pMM == 0 rows, overflows of x), the same with a gap-continuation byte of 0 on every 97th base (the plain form), the
    overflowing pair, and one pair each of 1 x 1, 192 rows (the longest read of the five-operation cell) and 193."""
    wide = whole_quality_range(synth, 600)
    gcp = wide["gcp"].copy()
    gcp[::97] = 0
    rng = np.random.RandomState(0xCE11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def pair(R, flank):
        read = rng.choice(acgt, R)
        hap = np.concatenate([rng.choice(acgt, flank), read, rng.choice(acgt, flank)])
        hap[flank + R // 2] = acgt[(int(np.searchsorted(acgt, read[R // 2])) + 1) % 4]       # one mismatch
        return one_pair(read, rng.randint(10, 41, R), rng.randint(30, 46, R), rng.randint(30, 46, R), rng.randint(5, 21, R), hap)

    return [("wide", wide), ("wide_gcp0", dict(wide, gcp=gcp)), ("overflow", overflowing_pair()),
            ("r1_h1", one_pair(b"C", 30, 40, 40, 10, b"C")), ("r192", pair(192, 14)), ("r193", pair(193, 14))]
