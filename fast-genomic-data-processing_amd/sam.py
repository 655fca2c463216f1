"""Host-side handle on the SAM text input C ABI (include/mgx_sam.h): the line framing, the shared rule set and its
completion by the full parser are host code (lines_host, encode_rules, encode_host); SamEncoder runs the same rule set on
the device.  Every encode returns an Encoded: line i's BAM record (block_size + record) is
bam[rec_off[i]:rec_off[i + 1]], empty where the rules declined the line (keys[i]["redo"] & REDO_DECLINED)."""
import ctypes as C
import errno
from collections import namedtuple

import numpy as np

from . import native
from .bam import KEY_DTYPE

MAX_LINE = 2048                 # MGX_SAM_MAX_LINE: the longest line the device encodes
REDO_DECLINED = 4               # MGX_SAM_REDO_DECLINED

Encoded = namedtuple("Encoded", "line_off line_len rec_off keys bam n_declined")


def out_bound(n_lines, n_text):
    """MGX_SAM_OUT_BOUND: the bytes of BAM that n_lines lines of n_text bytes can become"""
    return 36 * n_lines + 2 * n_text


class SamDataError(native.MgxError):
    """-EBADMSG of encode_host: the full parser rejected line `line`."""

    def __init__(self, msg, line):
        super().__init__(msg)
        self.line = line


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bytes(data):
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)


class SamTable:
    """mgx_sam_table_t: the header's reference names, in order."""

    def __init__(self, names):
        self.lib = native.load()
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        blob = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint32)
        h = C.c_void_p()
        native.check(self.lib.mgx_sam_table_create(len(raw), _ptr(blob), _ptr(off), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.lib.mgx_sam_table_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _table(t):
    return t if isinstance(t, SamTable) else SamTable(t)


def max_lines_of(n_text):
    return n_text // 2 + 1      # a line and its newline are at least two bytes


def lines_host(text):
    """-> (start, length) of every non-empty line (newline and one trailing CR not counted)"""
    lib = native.load()
    d = _bytes(text)
    cap = max_lines_of(len(d))
    off = np.zeros(cap, dtype=np.uint64); ln = np.zeros(cap, dtype=np.uint32)
    n = C.c_uint64()
    native.check(lib.mgx_sam_lines_host(_ptr(d), len(d), cap, _ptr(off), _ptr(ln), C.byref(n)))
    return off[:n.value].copy(), ln[:n.value].copy()


def _arrays(n_text, max_lines, out_capacity):
    max_lines = max_lines_of(n_text) if max_lines is None else max_lines
    cap = out_bound(max_lines, n_text) if out_capacity is None else out_capacity
    return (max_lines, cap, np.zeros(max(max_lines, 1), dtype=np.uint64), np.zeros(max(max_lines, 1), dtype=np.uint32),
            np.zeros(max_lines + 1, dtype=np.uint64), np.zeros(max(max_lines, 1), dtype=KEY_DTYPE), np.zeros(max(cap, 1), dtype=np.uint8))


def _encoded(off, ln, ro, keys, out, n, n_out, n_declined):
    n = int(n.value)
    return Encoded(off[:n].copy(), ln[:n].copy(), ro[:n + 1].copy(), keys[:n].copy(), out[:int(n_out.value)].copy(), int(n_declined.value))


def encode_rules(table, text, max_line=0, max_lines=None, out_capacity=None):
    """The shared rule set on the host: what the device must equal.  max_line: longer lines are declined (0: MAX_LINE)."""
    lib = native.load()
    t, d = _table(table), _bytes(text)
    max_lines, cap, off, ln, ro, keys, out = _arrays(len(d), max_lines, out_capacity)
    n, n_out, n_dec = C.c_uint64(), C.c_uint64(), C.c_uint64()
    native.check(lib.mgx_sam_encode_rules(t.h, _ptr(d), len(d), max_line, max_lines, cap, _ptr(off), _ptr(ln), _ptr(ro), _ptr(keys), _ptr(out),
                                          C.byref(n), C.byref(n_out), C.byref(n_dec)))
    return _encoded(off, ln, ro, keys, out, n, n_out, n_dec)


def encode_host(table, text, max_lines=None, out_capacity=None):
    """The rule set with every declined line completed by the full parser; a line that parser rejects raises SamDataError."""
    lib = native.load()
    t, d = _table(table), _bytes(text)
    max_lines, cap, off, ln, ro, keys, out = _arrays(len(d), max_lines, out_capacity)
    n, n_out, n_dec, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib.mgx_sam_encode_host(t.h, _ptr(d), len(d), max_lines, cap, _ptr(off), _ptr(ln), _ptr(ro), _ptr(keys), _ptr(out),
                                 C.byref(n), C.byref(n_out), C.byref(n_dec), C.byref(bad))
    if rc == -errno.EBADMSG:
        raise SamDataError(lib.mgx_last_error().decode(errors="replace"), int(bad.value))
    native.check(rc)
    return _encoded(off, ln, ro, keys, out, n, n_out, n_dec)


class SamEncoder:
    """The rule set on the device, on a BGZF context of its own.  encode() is the one-shot mgx_sam_encode; batch() gives a
    SamBatch for repeated submits."""

    def __init__(self, table, device=0):
        self.lib = native.load()
        self.table = _table(table)
        h = C.c_void_p()
        native.check(self.lib.mgx_bgzf_create(device, 0, C.byref(h)))
        self.h = h

    def encode(self, text, max_lines=None, out_capacity=None):
        d = _bytes(text)
        max_lines, cap, off, ln, ro, keys, out = _arrays(len(d), max_lines, out_capacity)
        n, n_out, n_dec = C.c_uint64(), C.c_uint64(), C.c_uint64()
        native.check(self.lib.mgx_sam_encode(self.h, self.table.h, _ptr(d), len(d), max_lines, cap, _ptr(off), _ptr(ln), _ptr(ro), _ptr(keys), _ptr(out),
                                             C.byref(n), C.byref(n_out), C.byref(n_dec)))
        return _encoded(off, ln, ro, keys, out, n, n_out, n_dec)

    def batch(self, text_capacity, max_records):
        return SamBatch(self, text_capacity, max_records)

    def stats(self):
        st = native.SamStats()
        native.check(self.lib.mgx_sam_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in native.SamStats._fields_}

    def close(self):
        if self.h:
            self.lib.mgx_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SamBatch:
    """mgx_sam_batch_t: pinned input, submit, wait."""

    def __init__(self, enc, text_capacity, max_records):
        self.enc, self.lib, self.cap, self.max_records = enc, enc.lib, text_capacity, max_records
        b = C.c_void_p()
        native.check(self.lib.mgx_sam_batch_create(enc.h, enc.table.h, text_capacity, max_records, C.byref(b)))
        self.b = b
        self.input = np.ctypeslib.as_array(C.cast(self.lib.mgx_sam_batch_input(b), C.POINTER(C.c_uint8)), shape=(max(text_capacity, 1),))

    def run(self, text, fetch=True):
        """submit + wait -> Encoded (bam empty with fetch=False: the records stay on the device, see device_records)"""
        d = _bytes(text)
        self.input[:len(d)] = d
        native.check(self.lib.mgx_sam_batch_submit(self.enc.h, self.b, len(d)))
        lo, ll, ro, k, bam = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, n_out = C.c_uint64(), C.c_uint64()
        native.check(self.lib.mgx_sam_batch_wait(self.enc.h, self.b, C.byref(lo), C.byref(ll), C.byref(ro), C.byref(k), C.byref(n), C.byref(n_out),
                                                 C.byref(bam) if fetch else None))
        m = int(n.value)

        def view(p, dt, cnt):
            if cnt == 0:
                return np.zeros(0, dtype=dt)
            return np.frombuffer((C.c_uint8 * (cnt * np.dtype(dt).itemsize)).from_address(p.value), dtype=dt).copy()
        keys = view(k, KEY_DTYPE, m)
        out = view(bam, np.uint8, int(n_out.value)) if fetch and n_out.value else np.zeros(0, dtype=np.uint8)
        return Encoded(view(lo, np.uint64, m), view(ll, np.uint32, m), view(ro, np.uint64, m + 1), keys, out,
                       int(np.count_nonzero(keys["redo"] & REDO_DECLINED)))

    def device_records(self):
        return int(self.lib.mgx_sam_batch_device_records(self.b))

    def close(self):
        if self.b:
            self.lib.mgx_sam_batch_destroy(self.enc.h, self.b)
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
