"""Host-side handle on the fused realignment C ABI (include/mgx_realign.h).

``RealignEngine.regions`` is Mutect2Engine's realignReadsToTheirBestHaplotype for several regions in one device call:
computeReadLikelihoods (``PairHMMEngine.regions``), then per kept read bestAllelesBreakingTies, the verbatim shortcut of
SWNativeAlignerWrapper and the aligner (``SmithWatermanEngine.align_batch``) of the read against its best haplotype.
"""
import ctypes as C

import numpy as np

from . import native
from .pairhmm import make_input
from .smithwaterman import SOFTCLIP

TO_BEST_HAPLOTYPE = (10, -15, -30, -5)      # ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS, read/CigarUtils.cpp:15
NOT_ALIGNED = native.REALIGN_NOT_ALIGNED


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


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
        native.check(self.lib.mgx_realign_regions(self.pairhmm.ctx, self.sw.ctx, n, C.cast(arr, C.c_void_p), cast("mapq"), C.byref(m),
                                                  None if priorities is None else cast("pri"), sp, strategy, cast("log10"), cast("keep"),
                                                  cast("best"), cast("offset"), cast("cigar"), stride, cast("score")))
        for o in res:
            cig = o["cigar"]
            lens = (cig != 0).sum(axis=1)                # the text holds no NUL before its end
            flat = cig.tobytes()
            o["cigar"] = [flat[p * stride:p * stride + int(lens[p])] for p in range(len(cig))]
            o.pop("mapq"); o.pop("pri", None)
        return res

    def stats(self):
        st = native.RealignStats()
        native.check(self.lib.mgx_realign_stats(self.pairhmm.ctx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}
