"""Host-side handle on the fused realignment C ABI (include/mgx_realign.h).

``RealignEngine.regions`` is Mutect2Engine's realignReadsToTheirBestHaplotype for several regions in one device call:
computeReadLikelihoods (``PairHMMEngine.regions``), then per kept read bestAllelesBreakingTies, the verbatim shortcut of
SWNativeAlignerWrapper and the aligner (``SmithWatermanEngine.align_batch``) of the read against its best haplotype.

``RealignEngine.to_ref`` and ``RealignEngine.regions_to_ref`` finish the stage: the read's start on the reference and its
read -> reference CIGAR (AlignmentUtils::createReadAlignedToRef behind its aligner call), as BAM-encoded elements.  Only the
SAMRecord clone is left to the caller.
"""
import ctypes as C

import numpy as np

from . import native
from .pairhmm import make_input
from .smithwaterman import SOFTCLIP

TO_BEST_HAPLOTYPE = (10, -15, -30, -5)      # ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS, read/CigarUtils.cpp:15
NOT_ALIGNED = native.REALIGN_NOT_ALIGNED


CIGAR_OPS = "MIDNSHP=X"


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def cigar_text(elements):
    """BAM-encoded elements (length << 4 | operator) as CIGAR text"""
    return "".join("%d%s" % (int(e) >> 4, CIGAR_OPS[int(e) & 15]) for e in elements)


def _csr(lists, dtype):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    flat = np.concatenate([np.asarray(x, dtype=dtype).ravel() for x in lists]) if len(lists) else np.zeros(0, dtype=dtype)
    return off, np.ascontiguousarray(flat if len(flat) else np.zeros(1, dtype=dtype), dtype=dtype)


def _bases(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, dtype=np.uint8)


class RealignEngine:
    """Joins a PairHMMEngine and a SmithWatermanEngine of the same device; owns neither."""

    def __init__(self, pairhmm_engine, sw_engine):
        self.lib = native.load()
        self.pairhmm, self.sw = pairhmm_engine, sw_engine

    def best_alleles(self, rows, priorities=None):
        """bestAllelesBreakingTies on rows of log10 likelihoods the caller holds: ``rows`` is a list of 1-d arrays (one per
        read), ``priorities`` a list of arrays of the same lengths or None (no tie-breaking).  Returns int32 [len(rows)]."""
        n = len(rows)
        nh = np.array([len(r) for r in rows], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(nh[:-1], dtype=np.uint64)
        flat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in xs]) if n else np.zeros(0))  # noqa: E731
        values = flat(rows)
        pri = None if priorities is None else flat(priorities)
        assert pri is None or len(pri) == len(values)
        best = np.zeros(n, dtype=np.int32)
        native.check(self.lib.mgx_pairhmm_best_alleles(self.pairhmm.ctx, n, _ptr(off), _ptr(nh), _ptr(values), None if pri is None else _ptr(pri),
                                                       _ptr(best)))
        return best

    def regions(self, regions, mapqs, priorities=None, params=None, strategy=SOFTCLIP, stride=None, **model_overrides):
        """Per region a dict: log10 [n_reads][n_haps], keep, best, offset (NOT_ALIGNED where keep == 0), cigar (list of bytes),
        score.  ``priorities``: None, or per region None or one double per haplotype.  ``params``: None = TO_BEST_HAPLOTYPE."""
        return self._regions(self.lib.mgx_realign_regions, (), regions, mapqs, priorities, params, strategy, stride, model_overrides)

    def _regions(self, fn, extra, regions, mapqs, priorities, params, strategy, stride, model_overrides):
        n = len(regions)
        arr = (native.PairHMMInput * n)()
        hold, res = [], []
        names = ("log10", "keep", "best", "offset", "cigar", "score", "mapq", "pri")
        P = {k: (C.c_void_p * n)() for k in names}
        longest = 1
        for g, d in enumerate(regions):
            d = dict(d); d["pair_read"] = None; d["pair_hap"] = None
            inp, keep = make_input(d)
            arr[g] = inp; hold.append(keep)
            for k in ("read_off", "hap_off"):
                longest = max(longest, int(np.diff(keep[k].astype(np.int64)).max(initial=1)))
        stride = 2 * longest + 1 if stride is None else stride
        for g in range(n):
            nr, nh = int(arr[g].n_reads), int(arr[g].n_haps)
            o = dict(log10=np.empty((nr, nh), dtype=np.float64), keep=np.zeros(nr, dtype=np.uint8), best=np.zeros(nr, dtype=np.int32),
                     offset=np.zeros(nr, dtype=np.int32), cigar=np.zeros((nr, stride), dtype=np.uint8), score=np.zeros(nr, dtype=np.int32),
                     mapq=np.ascontiguousarray(mapqs[g], dtype=np.uint8))
            if priorities is not None and priorities[g] is not None:
                o["pri"] = np.ascontiguousarray(priorities[g], dtype=np.float64)
                assert len(o["pri"]) == nh
            for k, a in o.items():
                P[k][g] = a.ctypes.data
            res.append(o)
        m = native.ReadModel()
        self.lib.mgx_read_model_defaults(C.byref(m))
        for k, v in model_overrides.items():
            setattr(m, k, v)
        sp = None if params is None else C.byref(native.SwParams(*params))
        cast = lambda k: C.cast(P[k], C.c_void_p)  # noqa: E731
        native.check(fn(self.pairhmm.ctx, self.sw.ctx, n, C.cast(arr, C.c_void_p), cast("mapq"), C.byref(m),
                        None if priorities is None else cast("pri"), sp, strategy, cast("log10"), cast("keep"),
                        cast("best"), cast("offset"), cast("cigar"), stride, cast("score"), *extra))
        for o in res:
            cig = o["cigar"]
            lens = (cig != 0).sum(axis=1)                # the text holds no NUL before its end
            flat = cig.tobytes()
            o["cigar"] = [flat[p * stride:p * stride + int(lens[p])] for p in range(len(cig))]
            o.pop("mapq"); o.pop("pri", None)
        return res

    def to_ref(self, reads, sw_offset, sw_cigars, read_hap, hap_cigars, hap_start, read_ref, refs, reference_start, hard_clips=None,
               stride=16):
        """createReadAlignedToRef behind its aligner call on alignments the caller holds.  ``reads`` and ``refs`` are lists of
        bytes / uint8 arrays, ``sw_cigars`` and ``hap_cigars`` lists of BAM-encoded uint32 element arrays; ``read_hap`` and
        ``read_ref`` index ``hap_cigars`` / ``hap_start`` and ``refs``; ``hard_clips`` is None or [n][2].  Returns
        (status uint8 [n], start int32 [n], cigars: a list of uint32 arrays, empty unless status == OK, n_cigar uint32 [n])."""
        n = len(reads)
        hold = {}
        hold["read_off"], hold["read_bases"] = _csr([_bases(x) for x in reads], np.uint8)
        hold["sw_cigar_off"], hold["sw_cigar"] = _csr(sw_cigars, np.uint32)
        hold["hap_cigar_off"], hold["hap_cigar"] = _csr(hap_cigars, np.uint32)
        hold["ref_off"], hold["ref_bases"] = _csr([_bases(x) for x in refs], np.uint8)
        for k, v, dt in (("sw_offset", sw_offset, np.int32), ("read_hap", read_hap, np.uint32), ("hap_start", hap_start, np.int32),
                         ("read_ref", read_ref, np.uint32), ("reference_start", reference_start, np.int32)):
            hold[k] = np.ascontiguousarray(v, dtype=dt)
            assert len(hold[k]) == (len(hap_cigars) if k == "hap_start" else n), k
        if hard_clips is not None:
            hold["hard_clips"] = np.ascontiguousarray(hard_clips, dtype=np.uint32).reshape(n, 2)
        inp = native.ToRefInput(n_reads=n, n_haps=len(hap_cigars), n_refs=len(refs), **{k: v.ctypes.data for k, v in hold.items()})
        start = np.zeros(n, dtype=np.int32); n_cigar = np.zeros(n, dtype=np.uint32); status = np.zeros(n, dtype=np.uint8)
        rows = np.zeros((n, stride), dtype=np.uint32)
        native.check(self.lib.mgx_read_to_ref(self.pairhmm.ctx, C.byref(inp), _ptr(start), _ptr(rows), stride, _ptr(n_cigar), _ptr(status)))
        cigars = [rows[r, :int(n_cigar[r])].copy() if status[r] == native.TO_REF_OK else np.zeros(0, np.uint32) for r in range(n)]
        return status, start, cigars, n_cigar

    def regions_to_ref(self, regions, mapqs, to_ref, priorities=None, params=None, strategy=SOFTCLIP, stride=None, ref_stride=16,
                       **model_overrides):
        """``regions`` and, per region, start, ref_cigar (a list of uint32 arrays), n_ref_cigar and status.  ``to_ref``: per region a
        dict with hap_cigars (a list of element arrays, one per haplotype), hap_start, ref_hap, reference_start and optionally
        hard_clips [n_reads][2]."""
        n = len(regions)
        tr = (native.ToRefRegion * max(n, 1))()
        hold, outs = [], []
        names = ("start", "rows", "n", "status")
        P = {k: (C.c_void_p * max(n, 1))() for k in names}
        for g, d in enumerate(to_ref):
            nr = len(regions[g]["read_off"]) - 1
            off, flat = _csr(d["hap_cigars"], np.uint32)
            hs = np.ascontiguousarray(d["hap_start"], dtype=np.int32)
            assert len(hs) == len(d["hap_cigars"]) == len(regions[g]["hap_off"]) - 1
            hc = None if d.get("hard_clips") is None else np.ascontiguousarray(d["hard_clips"], dtype=np.uint32).reshape(nr, 2)
            hold.append((off, flat, hs, hc))
            tr[g] = native.ToRefRegion(off.ctypes.data, flat.ctypes.data, hs.ctypes.data, int(d["ref_hap"]), int(d["reference_start"]),
                                       None if hc is None else hc.ctypes.data)
            o = dict(start=np.zeros(nr, dtype=np.int32), rows=np.zeros((nr, ref_stride), dtype=np.uint32), n=np.zeros(nr, dtype=np.uint32),
                     status=np.zeros(nr, dtype=np.uint8))
            for k in names:
                P[k][g] = o[k].ctypes.data
            outs.append(o)
        cast = lambda k: C.cast(P[k], C.c_void_p)  # noqa: E731
        extra = (C.cast(tr, C.c_void_p), cast("start"), cast("rows"), ref_stride, cast("n"), cast("status"))
        res = self._regions(self.lib.mgx_realign_regions_to_ref, extra, regions, mapqs, priorities, params, strategy, stride, model_overrides)
        for o, t in zip(res, outs):
            o["start"], o["status"], o["n_ref_cigar"] = t["start"], t["status"], t["n"]
            o["ref_cigar"] = [t["rows"][r, :int(t["n"][r])].copy() if t["status"][r] == native.TO_REF_OK else np.zeros(0, np.uint32)
                              for r in range(len(t["n"]))]
        return res

    def to_ref_stats(self):
        st = native.RealignToRefStats()
        native.check(self.lib.mgx_realign_to_ref_stats(self.pairhmm.ctx, C.byref(st)))
        return {"n_status": [int(x) for x in st.n_status], "ms_to_ref": float(st.ms_to_ref)}

    def stats(self):
        st = native.RealignStats()
        native.check(self.lib.mgx_realign_stats(self.pairhmm.ctx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}
