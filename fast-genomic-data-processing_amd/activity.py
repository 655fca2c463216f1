"""Host-side handle on the active-site detection C ABI (include/mgx_activity.h).

``ActivityEngine.interval`` is Mutect2Engine::isActive for every locus of one contig interval: per (read, locus) the alt
quality of the read's pileup element, per locus the tumour log-odds, the normal's veto and the 0 / 1 activity value.  The
read filters, the down-sampler, the pileup windows and everything behind the per-locus value stay with the caller.
"""
import ctypes as C

import numpy as np

from . import native

TIMING = 2      # MGX_PAIRHMM_TIMING
READ_FIELDS = (("read_start", np.int32), ("flags", np.uint16), ("mate_start", np.int32), ("sample", np.uint8), ("act_start", np.int32),
               ("act_stop", np.int32))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def make_input(d):
    """``d``: interval_start, ref_bases (uint8 [n_loci]) and per read read_start, cigar_off / cigar (BAM-encoded uint32), base_off /
    bases / quals, flags, mate_start, sample, act_start, act_stop.  Returns (ActivityInput, the arrays it points into)."""
    hold = {"ref_bases": np.ascontiguousarray(d["ref_bases"], dtype=np.uint8)}
    for k, dt in READ_FIELDS + (("cigar_off", np.uint64), ("cigar", np.uint32), ("base_off", np.uint64), ("bases", np.uint8), ("quals", np.uint8)):
        hold[k] = np.ascontiguousarray(d[k], dtype=dt)
    n = len(hold["read_start"])
    for k, _ in READ_FIELDS:
        assert len(hold[k]) == n, k
    assert len(hold["cigar_off"]) == n + 1 and len(hold["base_off"]) == n + 1 and len(hold["bases"]) == len(hold["quals"])
    inp = native.ActivityInput(interval_start=int(d["interval_start"]), n_loci=len(hold["ref_bases"]), n_reads=n,
                               **{k: v.ctypes.data for k, v in hold.items()})
    return inp, hold


class ActivityEngine:
    def __init__(self, device=0, max_depth=0):
        self.lib = native.load()
        self.ctx = C.c_void_p()
        native.check(self.lib.mgx_activity_create(device, max_depth, C.byref(self.ctx)))

    def params(self, **overrides):
        p = native.ActivityParams()
        self.lib.mgx_activity_params_defaults(C.byref(p))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p

    def interval_rc(self, d, **params):
        """The call's return code and its outputs (active uint8, log_odds float64, depth uint32), without raising."""
        inp, hold = make_input(d)
        n = int(inp.n_loci)
        active = np.full(n, 255, dtype=np.uint8); log_odds = np.full(n, -1.0); depth = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        rc = self.lib.mgx_activity_interval(self.ctx, C.byref(inp), C.byref(self.params(**params)), _ptr(active), _ptr(log_odds), _ptr(depth))
        del hold
        return rc, active, log_odds, depth

    def interval(self, d, **params):
        rc, active, log_odds, depth = self.interval_rc(d, **params)
        native.check(rc)
        return active, log_odds, depth

    def stats(self):
        st = native.ActivityStats()
        native.check(self.lib.mgx_activity_stats(self.ctx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}

    def last_elements(self):
        """the element bytes of the last interval call: per read, in input order, one byte per position of its window"""
        out = np.zeros(int(self.stats()["n_elements"]), dtype=np.uint8)
        native.check(self.lib.mgx_activity_last_elements(self.ctx, _ptr(out), len(out)))
        return out

    def close(self):
        if self.ctx:
            self.lib.mgx_activity_destroy(self.ctx)
            self.ctx = C.c_void_p()
