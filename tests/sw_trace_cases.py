"""Inputs of the Smith-Waterman back-trace tests (tests/test_sw_trace_host.py on the CPU, tests/test_sw_trace_gpu.py on the device): one
family of pairs per seam of csrc/sw_trace_rule.h and of k_sw_trace_wave.  Plain numpy, regenerated from seeds; expected values are the
oracle's, never stored here.  A case is a dict(family, name, ref, alt, params, strategy, caps, want) -- `want` holds what the host test
asserts of the driver's counters or of the answer, so that a family that stops reaching its seam fails instead of passing idly:
  run         the longest match run the 64-lane walk consumed in one step
  refetches   at least this many fetches of a diagonal
  candidates  at least this many end-cell candidates (cells that hold the maximum, on the edges the strategy uses)
  n_elems     merged elements of the alignment
  text        the CIGAR text (where the construction fixes it)"""
import numpy as np

import sw_long as L

STANDARD_NGS, ORIGINAL_DEFAULT = (25, -50, -110, -6), (3, -1, -4, -3)
SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 9, 10, 11, 12
STRATEGIES = (SOFTCLIP, INDEL, LEADING_INDEL, IGNORE)
FAMILIES = ("register_seam", "match_run", "run_boundary", "bounded_run", "tie", "elements", "degenerate", "long_ref", "random")
COMPACT_ELEMS = 16          # kCompactElems of csrc/mgx_smithwaterman.hip
EDGE_CELLS = 512            # 64 * kEdgeRegs: up to here both edges fit the trace kernel's registers


def _b(text):
    return np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8).copy()


def _acg(rng, n):
    """random bases without T: a T placed by the builder matches nothing by accident"""
    return _b("ACG")[rng.integers(0, 3, n)]


def _case(family, name, ref, alt, strategy, params=STANDARD_NGS, caps=(), **want):
    return dict(family=family, name=f"{family}/{name}/{strategy}", ref=np.ascontiguousarray(ref, dtype=np.uint8),
                alt=np.ascontiguousarray(alt, dtype=np.uint8), params=params, strategy=strategy, caps=tuple(caps), want=want)


def register_seam():
    """len1 + len2 around 512, where the edges stop fitting the registers and the two-pass end cell takes over"""
    out = []
    for q, (n, m) in enumerate(((256, 255), (256, 256), (257, 256), (500, 12), (12, 500))):
        ref, alt = L.make_pair(n, m, 4100 + q)
        out += [_case("register_seam", f"{n}x{m}", ref, alt, st) for st in STRATEGIES]
    return out


def match_runs():
    """identical sequences: the whole alignment is one run, consumed 64 cells at a time; a run of 64 or 128 ends exactly at a refetch"""
    out = []
    for n in (63, 64, 65, 127, 128, 129):
        s = L.random_bases(np.random.default_rng(4200 + n), n)
        out += [_case("match_run", f"identical{n}", s, s, st, run=min(n, 64), refetches=-(-n // 64), text=f"{n}M") for st in STRATEGIES]
    return out


def run_boundaries():
    """one mismatch, insertion or deletion whose first cell is lane 0, 1, 62 or 63 of the first cached diagonal: `p` matching bases
    follow it.  Flanks without T, the variant all T: its place is unique.  INDEL walks from the corner, so the text is fixed; a
    mismatch is a diagonal step and does not end a run.  Then gaps longer than a diagonal of 64 cells."""
    out = []
    rng = np.random.default_rng(4300)
    for p in (0, 1, 62, 63):
        pre, suf = _acg(rng, 70), _acg(rng, p)
        T = _b("TTT")
        out.append(_case("run_boundary", f"mismatch@{p}", np.concatenate([pre, _b("A"), suf]), np.concatenate([pre, _b("T"), suf]), INDEL,
                         refetches=2, run=64, text=f"{71 + p}M"))
        out.append(_case("run_boundary", f"insertion@{p}", np.concatenate([pre, suf]), np.concatenate([pre, T, suf]), INDEL,
                         refetches=2, run=64, text=f"70M3I{p}M" if p else "70M3I"))
        out.append(_case("run_boundary", f"deletion@{p}", np.concatenate([pre, T, suf]), np.concatenate([pre, suf]), INDEL,
                         refetches=2, run=64, text=f"70M3D{p}M" if p else "70M3D"))
    pre, suf, gap = _acg(rng, 50), _acg(rng, 50), np.full(70, ord("T"), np.uint8)
    for st in (SOFTCLIP, INDEL):
        out.append(_case("run_boundary", "deletion70", np.concatenate([pre, gap, suf]), np.concatenate([pre, suf]), st, refetches=2, run=50, text="50M70D50M"))
        out.append(_case("run_boundary", "insertion70", np.concatenate([pre, suf]), np.concatenate([pre, gap, suf]), st, refetches=2, run=50, text="50M70I50M"))
    return out


def bounded_runs():
    """the run is bounded by j or by i: fewer than 64 cells of the diagonal lie inside the matrix, the lanes beyond it hold 0 = a match"""
    rng = np.random.default_rng(4400)
    ref = _acg(rng, 100)
    out = [_case("bounded_run", "by_j", ref, ref[30:60], st, run=30) for st in STRATEGIES]
    short = _acg(rng, 20)
    out += [_case("bounded_run", "by_i", short, np.concatenate([np.full(30, ord("T"), np.uint8), short]), st, run=20) for st in STRATEGIES]
    return out


def ties():
    """the maximum more than once on the last row, on the last column, on both at differing |i - j|, and in the corner"""
    motif = "ACGT"
    pairs = (("row", motif * 3, motif * 8), ("row_two_blocks", motif * 3, motif * 30), ("col", motif * 8, motif * 3),
             ("col_two_blocks", motif * 30, motif * 3), ("corner", motif * 4, motif * 4),
             ("both_same_diagonal", "GCCCA", "ATTTG"), ("both_col_first", "GCCCCCA", "ATTTG"), ("both_row_first", "GCCCA", "ATTTTTG"),
             ("both_many", "GCACA", "ATGTG"))
    out = []
    for name, ref, alt in pairs:
        for params in (STANDARD_NGS, ORIGINAL_DEFAULT):
            for st in STRATEGIES:
                want = dict(candidates=2) if st in (SOFTCLIP, IGNORE) else {}
                out.append(_case("tie", f"{name}/{params[0]}", _b(ref), _b(alt), st, params, **want))
    return out


def element_lists():
    """exactly 15, 16, 17 and 40 merged elements (INDEL: no clip), around the 16 the trace kernel copies back per pair; also under text
    buffers too small for all of them.  Segments of 12 matches without T, between them a TT inserted or deleted in turn; an even count
    comes from four unmatched bases in front of the alternate."""
    out = []
    for n_elems in (15, 16, 17, 40):
        rng = np.random.default_rng(4500 + n_elems)
        k = (n_elems + 1) // 2
        ref, alt = [], ([_b("TTTT")] if n_elems % 2 == 0 else [])
        for s in range(k):
            seg = _acg(rng, 12)
            ref.append(seg); alt.append(seg)
            if s + 1 < k:
                (alt if s % 2 else ref).append(_b("TT"))
        for st in STRATEGIES:
            want = dict(n_elems=n_elems) if st == INDEL else {}
            out.append(_case("elements", f"{n_elems}", np.concatenate(ref), np.concatenate(alt), st, caps=(3, 6), **want))
    return out


def degenerate():
    rng = np.random.default_rng(4600)
    long = _acg(rng, 300)
    out = []
    for st in STRATEGIES:
        out.append(_case("degenerate", "1x1", _b("A"), _b("A"), st))
        out.append(_case("degenerate", "1x1_mismatch", _b("A"), _b("C"), st))
        out.append(_case("degenerate", "1x300", long[150:151], long, st))
        out.append(_case("degenerate", "300x1", long, long[150:151], st))
        out.append(_case("degenerate", "all_mismatch", np.full(20, ord("A"), np.uint8), np.full(15, ord("C"), np.uint8), st))
    tail = _acg(rng, 20)
    out.append(_case("degenerate", "indel_ends_i>0", np.concatenate([_acg(rng, 30), tail]), tail, INDEL, text="30D20M"))
    out.append(_case("degenerate", "indel_ends_j>0", tail, np.concatenate([np.full(30, ord("T"), np.uint8), tail]), INDEL, text="30I20M"))
    return out


def long_refs():
    """references beyond one strip of 2048 rows: BtView adds the strip term"""
    out = []
    for q, (n, m) in enumerate(((2049, 40), (4097, 65))):
        ref, alt = L.make_pair(n, m, 4700 + q)
        out += [_case("long_ref", f"{n}x{m}", ref, alt, st) for st in STRATEGIES]
    return out


def random_pairs(n=300):
    rng = np.random.default_rng(4800)
    out = []
    for q in range(n):
        l1, l2 = int(rng.integers(1, 131)), int(rng.integers(1, 161))
        ref = L.random_bases(rng, l1)
        if q % 3 == 0:
            alt = L.random_bases(rng, l2)
        else:                               # a piece of the reference with substitutions and short indels, random flanks up to l2
            a = int(rng.integers(0, l1)); piece = list(ref[a:a + l2])
            for _ in range(int(rng.integers(0, 4))):
                at = int(rng.integers(0, len(piece) + 1)); kind = int(rng.integers(0, 3)); k = int(rng.integers(1, 5))
                if kind == 0:
                    piece[at:at + k] = []
                elif kind == 1:
                    piece[at:at] = list(L.random_bases(rng, k))
                elif at < len(piece):
                    piece[at] = int(L.random_bases(rng, 1)[0])
            flank = L.random_bases(rng, max(l2 - len(piece), 0))
            cut = int(rng.integers(0, len(flank) + 1))
            alt = np.concatenate([flank[:cut], np.array(piece, dtype=np.uint8), flank[cut:]])[:l2]
        out.append(_case("random", f"{q}", ref, alt, STRATEGIES[q % 4], (STANDARD_NGS, ORIGINAL_DEFAULT)[(q // 4) % 2]))
    return out


def all_cases():
    return register_seam() + match_runs() + run_boundaries() + bounded_runs() + ties() + element_lists() + degenerate() + long_refs() + random_pairs()


def expected(sw_oracle, cases):
    """per case: (text, offset, score, {cap: text under that capacity})"""
    out = []
    for c in cases:
        text, off, score = sw_oracle.align(c["ref"], c["alt"], c["params"], c["strategy"])
        out.append((text, off, score, {cap: sw_oracle.align(c["ref"], c["alt"], c["params"], c["strategy"], cap=cap)[0] for cap in c["caps"]}))
    return out
