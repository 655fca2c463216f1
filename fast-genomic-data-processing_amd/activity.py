"""Host-side handle on the active-site detection C ABI (include/mgx_activity.h).

``ActivityEngine.interval`` is Mutect2Engine::isActive for every locus of one contig interval: per (read, locus) the alt
quality of the read's pileup element, per locus the tumour log-odds, the normal's veto and the 0 / 1 activity value.  The
read filters, the down-sampler, the pileup windows and everything behind the per-locus value stay with the caller.
"""
import ctypes as C

import numpy as np

from . import native

TIMING = 2      # MGX_PAIRHMM_TIMING
BAND_TILE, MAX_FILTER = 256, 256      # MGX_ACTIVITY_BAND_TILE, MGX_ACTIVITY_MAX_FILTER
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

    def region_params(self, weights=None, **overrides):
        """(ActivityRegionParams, the weight array it points into)"""
        rp = native.ActivityRegionParams()
        self.lib.mgx_activity_region_params_defaults(C.byref(rp))
        for k, v in overrides.items():
            setattr(rp, k, v)
        hold = None
        if weights is not None:
            hold = np.ascontiguousarray(weights, dtype=np.float64)
            rp.band_weights, rp.n_band_weights = hold.ctypes.data, len(hold)
        return rp, hold

    def band_weights(self, weights=None, **overrides):
        """(the 2F + 1 weights a region call with these parameters uses, F); host only"""
        rp, hold = self.region_params(weights, **overrides)
        out, f = np.zeros(2 * MAX_FILTER + 1), C.c_int32(-1)
        native.check(self.lib.mgx_activity_band_weights(C.byref(rp), _ptr(out), len(out), C.byref(f)))
        del hold
        return out[:2 * f.value + 1].copy(), int(f.value)

    def profile_regions_rc(self, interval_start, prob, contig_length, weights=None, cap=None, profile=True, profile_cap=None, **overrides):
        """The return code, the regions (int32 [n, 4]: start, end, ext_start, ext_end), the state values (or None), the counts the call
        reported (n_regions, n_states); without raising."""
        prob = np.ascontiguousarray(prob, dtype=np.float64)
        rp, hold = self.region_params(weights, **overrides)
        cap = len(prob) + 1 if cap is None else cap
        profile_cap = len(prob) + MAX_FILTER if profile_cap is None else profile_cap
        regions = np.full((max(cap, 1), 4), -1, dtype=np.int32)
        values = np.full(max(profile_cap, 1), -1.0) if profile else None
        n_regions, n_states = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.mgx_activity_profile_regions(self.ctx, int(interval_start), len(prob), _ptr(prob), int(contig_length), C.byref(rp), _ptr(regions), cap,
                                                   C.byref(n_regions), _ptr(values) if profile else None, profile_cap, C.byref(n_states))
        del hold
        return rc, regions, values, (int(n_regions.value), int(n_states.value))

    def profile_regions(self, interval_start, prob, contig_length, weights=None, profile=True, **overrides):
        rc, regions, values, (n_regions, n_states) = self.profile_regions_rc(interval_start, prob, contig_length, weights, profile=profile, **overrides)
        native.check(rc)
        return regions[:n_regions].copy(), (values[:n_states].copy() if profile else None)

    def interval_regions_rc(self, d, contig_length, weights=None, per_locus=True, profile=True, cap=None, region_params=None, **params):
        """Reads to regions in one call.  The return code, the regions, the state values (or None), (active, log_odds, depth) (or None),
        the counts (n_regions, n_states); without raising.  ``params`` are the per-locus parameters, ``region_params`` the regions'."""
        inp, hold = make_input(d)
        n = int(inp.n_loci)
        rp, hold_w = self.region_params(weights, **(region_params or {}))
        cap = n + 1 if cap is None else cap
        regions = np.full((max(cap, 1), 4), -1, dtype=np.int32)
        values = np.full(n + MAX_FILTER + 1, -1.0) if profile else None
        loci = (np.full(n, 255, dtype=np.uint8), np.full(n, -1.0), np.full(n, 0xFFFFFFFF, dtype=np.uint32)) if per_locus else None
        n_regions, n_states = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.mgx_activity_interval_regions(self.ctx, C.byref(inp), C.byref(self.params(**params)), int(contig_length), C.byref(rp), _ptr(regions), cap,
                                                    C.byref(n_regions), _ptr(values) if profile else None, len(values) if profile else 0, C.byref(n_states),
                                                    *([_ptr(a) for a in loci] if per_locus else [None, None, None]))
        del hold, hold_w
        return rc, regions, values, loci, (int(n_regions.value), int(n_states.value))

    def interval_regions(self, d, contig_length, weights=None, per_locus=True, profile=True, region_params=None, **params):
        rc, regions, values, loci, (n_regions, n_states) = self.interval_regions_rc(d, contig_length, weights, per_locus, profile, None, region_params, **params)
        native.check(rc)
        return regions[:n_regions].copy(), (values[:n_states].copy() if profile else None), loci

    def region_stats(self):
        st = native.ActivityRegionStats()
        native.check(self.lib.mgx_activity_region_stats(self.ctx, C.byref(st)))
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
