"""Host-side handle on the BAM input C ABI (include/mgx_bam.h): the header, the serial record walk and the keys are host
code (parse_header, walk_host, keys_host, keys_redo, pack_keys); BamScanner finds the same record starts and keys on the
device."""
import ctypes as C
import errno

import numpy as np

from . import native
from .synth import REC_DTYPE

KEY_DTYPE = np.dtype([("d5", "<i8"), ("tid", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("flag", "<u2"), ("score", "<u2"),
                      ("tile", "<u2"), ("x", "<u2"), ("y", "<u2"), ("same_qname", "u1"), ("redo", "u1")])
assert KEY_DTYPE.itemsize == 32 == C.sizeof(native.BamKey)
MIN_RECORD = 37                 # 4 + the smallest block_size that holds a name: bounds the records of n bytes
PARTIAL = 1


class BamDataError(native.MgxError):
    """-EBADMSG: a corrupt record on the chain; n_records records precede it, next is its offset."""

    def __init__(self, msg, n_records, next):
        super().__init__(msg)
        self.n_records, self.next = n_records, next


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bytes(data):
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)


def parse_header(data):
    """-> (text, [(name, length)], offset of the first record), or None when `data` ends inside the header."""
    lib = native.load()
    d = _bytes(data)
    h = native.BamHeader()
    rc = lib.mgx_bam_parse_header(_ptr(d), len(d), C.byref(h), 0, None, None, None)
    if rc == PARTIAL:
        return None
    native.check(rc)
    n_ref = int(h.n_ref)
    off = np.zeros(max(n_ref, 1), dtype=np.uint64); ln = np.zeros(max(n_ref, 1), dtype=np.uint32); rl = np.zeros(max(n_ref, 1), dtype=np.uint32)
    native.check(lib.mgx_bam_parse_header(_ptr(d), len(d), C.byref(h), n_ref, _ptr(off), _ptr(ln), _ptr(rl)))
    raw = d.tobytes()
    refs = [(raw[int(off[i]):int(off[i]) + int(ln[i])].decode(), int(rl[i])) for i in range(n_ref)]
    return raw[int(h.text_off):int(h.text_off + h.text_len)].decode(), refs, int(h.first)


def walk_host(data, first, n=None):
    """The serial chain walk over data[:n] -> (record offsets, next).  A corrupt record raises BamDataError."""
    lib = native.load()
    d = _bytes(data)
    n = len(d) if n is None else n
    cap = max(0, n - min(first, n)) // MIN_RECORD + 1
    off = np.zeros(cap, dtype=np.uint64)
    cnt, nxt = C.c_uint64(), C.c_uint64()
    rc = lib.mgx_bam_walk_host(_ptr(d), n, first, cap, _ptr(off), C.byref(cnt), C.byref(nxt))
    if rc == -errno.EBADMSG:
        raise BamDataError(lib.mgx_last_error().decode(), int(cnt.value), int(nxt.value))
    native.check(rc)
    return off[:int(cnt.value)].copy(), int(nxt.value)


def keys_host(data, rec_off, rules_only=False):
    """Complete keys; rules_only: as the rule set shared with the device leaves them, redo bits set."""
    lib = native.load()
    d = _bytes(data)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    keys = np.zeros(len(rec_off), dtype=KEY_DTYPE)
    fn = lib.mgx_bam_keys_rules if rules_only else lib.mgx_bam_keys_host
    native.check(fn(_ptr(d), _ptr(rec_off), len(rec_off), _ptr(keys)))
    return keys


def keys_redo(data, rec_off, keys):
    """Device-made keys with their redo bits -> complete keys (a copy)."""
    lib = native.load()
    d = _bytes(data)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    keys = np.array(keys, dtype=KEY_DTYPE)
    native.check(lib.mgx_bam_keys_redo(_ptr(d), _ptr(rec_off), len(rec_off), _ptr(keys)))
    return keys


def pack_keys(keys, target_len):
    """sortdedup.pack for keys -> (recs [arrival order, REC_DTYPE], input_index, L)."""
    lib = native.load()
    keys = np.ascontiguousarray(keys, dtype=KEY_DTYPE)
    tl = np.ascontiguousarray(target_len, dtype=np.uint64)
    recs = np.zeros(len(keys), dtype=REC_DTYPE)
    idx = np.zeros(len(keys), dtype=np.uint32)
    L = C.c_uint64()
    native.check(lib.mgx_bam_pack_keys(len(keys), _ptr(keys), len(tl), _ptr(tl), _ptr(recs), _ptr(idx), C.byref(L)))
    return recs, idx, int(L.value)


class BamScanner:
    """mgx_bam_scan on a context of its own: inflated BAM bytes -> record offsets and keys, on the device."""

    def __init__(self, device=0):
        self.lib = native.load()
        h = C.c_void_p()
        native.check(self.lib.mgx_bgzf_create(device, 0, C.byref(h)))
        self.h = h

    def scan(self, data, first, n_ref, n=None, max_records=None):
        """-> (record offsets, keys with their redo bits, next).  A corrupt record raises BamDataError."""
        d = _bytes(data)
        n = len(d) if n is None else n
        cap = max(0, n - min(first, n)) // MIN_RECORD + 1 if max_records is None else max_records
        off = np.zeros(max(cap, 1), dtype=np.uint64)
        keys = np.zeros(max(cap, 1), dtype=KEY_DTYPE)
        cnt, nxt = C.c_uint64(), C.c_uint64()
        rc = self.lib.mgx_bam_scan(self.h, _ptr(d), n, first, n_ref, cap, _ptr(off), _ptr(keys), C.byref(cnt), C.byref(nxt))
        if rc == -errno.EBADMSG:
            raise BamDataError(self.lib.mgx_last_error().decode(), int(cnt.value), int(nxt.value))
        native.check(rc)
        k = int(cnt.value)
        return off[:k].copy(), keys[:k].copy(), int(nxt.value)

    def stats(self):
        st = native.BamStats()
        native.check(self.lib.mgx_bam_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in native.BamStats._fields_}

    def close(self):
        if self.h:
            self.lib.mgx_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
