"""Host-side handle on the BGZF C ABI (include/mgx_bgzf.h): the compressor and the inflater run on the device only; the
block scanner (scan_blocks) is host code."""
import ctypes as C
import errno

import numpy as np

from . import native

MAX_BLOCK_IN = 0xff00
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class BgzfCompressor:
    """mgx_bgzf_t: pieces of a byte stream -> BGZF blocks (bgzf_compress, htslib bgzf.c:610, on the device)."""

    def __init__(self, device=0, flags=0):
        self.lib = native.load()
        h = C.c_void_p()
        native.check(self.lib.mgx_bgzf_create(device, flags, C.byref(h)))
        self.h = h

    def compress(self, data, offsets=None, block=MAX_BLOCK_IN):
        """data: bytes-like; offsets: block boundaries (default: every `block` bytes).
        Returns (blocks back to back as a uint8 array, offsets of the blocks in it)."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        if offsets is None:
            offsets = np.arange(0, len(data) + block, block, dtype=np.uint64)
            offsets[-1] = len(data)
            if len(offsets) >= 2 and offsets[-2] == offsets[-1] and len(data):
                offsets = offsets[:-1]
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nb = len(offsets) - 1
        cap = int(self.lib.mgx_bgzf_bound(int(offsets[-1] - offsets[0]), nb))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(nb + 1, dtype=np.uint64)
        native.check(self.lib.mgx_bgzf_compress(self.h, _ptr(data), _ptr(offsets), nb, _ptr(out), cap, _ptr(out_off)))
        return out[: int(out_off[-1])], out_off

    def stats(self):
        st = native.BgzfStats()
        native.check(self.lib.mgx_bgzf_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in native.BgzfStats._fields_}

    def close(self):
        if self.h:
            self.lib.mgx_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BgzfBatch:
    """mgx_bgzf_batch_t: a pinned input buffer filled in place, submitted, waited for."""

    def __init__(self, comp, in_capacity, max_blocks):
        self.comp = comp
        self.lib = comp.lib
        b = C.c_void_p()
        native.check(self.lib.mgx_bgzf_batch_create(comp.h, in_capacity, max_blocks, C.byref(b)))
        self.b = b
        self.in_capacity, self.max_blocks = in_capacity, max_blocks
        self.input = np.ctypeslib.as_array(C.cast(self.lib.mgx_bgzf_batch_input(b), C.POINTER(C.c_uint8)), shape=(in_capacity,))
        self.offsets = np.ctypeslib.as_array(C.cast(self.lib.mgx_bgzf_batch_offsets(b), C.POINTER(C.c_uint64)), shape=(max_blocks + 1,))
        self.n_blocks = 0

    def submit(self, n_blocks):
        native.check(self.lib.mgx_bgzf_batch_submit(self.comp.h, self.b, n_blocks))
        self.n_blocks = n_blocks

    def wait(self):
        out, off = C.c_void_p(), C.c_void_p()
        native.check(self.lib.mgx_bgzf_batch_wait(self.comp.h, self.b, C.byref(out), C.byref(off)))
        o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(self.n_blocks + 1,)).copy()
        total = int(o[-1])
        data = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(max(total, 1),))[:total].copy()
        return data, o

    def close(self):
        if self.b:
            self.lib.mgx_bgzf_batch_destroy(self.comp.h, self.b)
            self.b = None


class BgzfStore:
    """mgx_bgzf_store_t: records resident in HBM (put), emitted as a sorted, duplicate-marked BGZF stream (emit)."""

    def __init__(self, comp):
        self.comp = comp
        self.lib = comp.lib
        h = C.c_void_p()
        native.check(self.lib.mgx_bgzf_store_create(comp.h, C.byref(h)))
        self.h = h

    def put(self, data):
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        addr = C.c_uint64()
        native.check(self.lib.mgx_bgzf_store_put(self.h, _ptr(data), len(data), C.byref(addr)))
        return int(addr.value)

    def put_device(self, device_ptr, n_bytes):
        """n_bytes that lie in device memory (SamBatch.device_records() after a run) -> their address in the store"""
        addr = C.c_uint64()
        native.check(self.lib.mgx_bgzf_store_put_device(self.h, device_ptr, n_bytes, C.byref(addr)))
        return int(addr.value)

    def emit(self, order, dup, addr, length):
        """Returns (all blocks back to back as bytes, compressed offset of every block, uoff[n + 1])."""
        order = np.ascontiguousarray(order, dtype=np.uint32); dup = np.ascontiguousarray(dup, dtype=np.uint8)
        addr = np.ascontiguousarray(addr, dtype=np.uint64); length = np.ascontiguousarray(length, dtype=np.uint32)
        n = len(order)
        uoff = np.zeros(n + 1, dtype=np.uint64)
        parts, block_at = [], []
        total = [0]

        def sink(_user, blocks, n_bytes, n_blocks, block_off):
            parts.append(C.string_at(blocks, n_bytes))
            oo = np.ctypeslib.as_array(C.cast(block_off, C.POINTER(C.c_uint64)), shape=(n_blocks + 1,))
            block_at.extend(int(total[0] + x) for x in oo[:n_blocks])
            total[0] += int(n_bytes)
            return 0
        cb = native.BGZF_SINK(sink)
        native.check(self.lib.mgx_bgzf_store_emit(self.h, n, _ptr(order), _ptr(dup), _ptr(addr), _ptr(length), cb, None, _ptr(uoff)))
        return b"".join(parts), np.array(block_at + [total[0]], dtype=np.uint64), uoff

    def close(self):
        if self.h:
            self.lib.mgx_bgzf_store_destroy(self.h)
            self.h = None


SCAN_END, SCAN_PARTIAL, SCAN_NOT_BGZF, SCAN_FULL = 0, 1, 2, 3


def scan_blocks(data, max_blocks=None):
    """mgx_bgzf_scan_blocks (host only): (block offsets [n + 1], ISIZEs [n], CRCs [n], stop reason)."""
    lib = native.load()
    data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    if max_blocks is None:
        max_blocks = len(data) // 26 + 1
    off = np.zeros(max_blocks + 1, dtype=np.uint64)
    isize = np.zeros(max(max_blocks, 1), dtype=np.uint32)
    crc = np.zeros(max(max_blocks, 1), dtype=np.uint32)
    n, stop = C.c_uint64(), C.c_int()
    native.check(lib.mgx_bgzf_scan_blocks(_ptr(data), len(data), max_blocks, _ptr(off), _ptr(isize), _ptr(crc), C.byref(n), C.byref(stop)))
    k = int(n.value)
    return off[:k + 1], isize[:k], crc[:k], int(stop.value)


class BgzfInflater:
    """The inflate side of mgx_bgzf_t: BGZF blocks -> their bytes, one wavefront per block on the device."""

    def __init__(self, device=0):
        self.lib = native.load()
        h = C.c_void_p()
        native.check(self.lib.mgx_bgzf_create(device, 0, C.byref(h)))
        self.h = h

    def decompress(self, data):
        """Whole BGZF blocks (pageable memory, one shot) -> bytes."""
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        _, isize, _, _ = scan_blocks(data)
        total = int(isize.sum(dtype=np.uint64))
        out = np.empty(max(total, 1), dtype=np.uint8)
        n = C.c_uint64()
        native.check(self.lib.mgx_bgzf_decompress(self.h, _ptr(data), len(data), _ptr(out), total, C.byref(n)))
        return out[: int(n.value)].tobytes()

    def batch(self, in_capacity, out_capacity, max_blocks):
        return InflateBatch(self, in_capacity, out_capacity, max_blocks)

    def stats(self):
        st = native.BgzfInflateStats()
        native.check(self.lib.mgx_bgzf_inflate_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in native.BgzfInflateStats._fields_}

    def close(self):
        if self.h:
            self.lib.mgx_bgzf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class InflateBatch:
    """mgx_bgzf_inflate_t: whole blocks into the pinned input (fill), submit, wait."""

    def __init__(self, inf, in_capacity, out_capacity, max_blocks):
        self.inf, self.lib = inf, inf.lib
        b = C.c_void_p()
        native.check(self.lib.mgx_bgzf_inflate_batch_create(inf.h, in_capacity, out_capacity, max_blocks, C.byref(b)))
        self.b = b
        self.in_capacity, self.out_capacity, self.max_blocks = in_capacity, out_capacity, max_blocks
        self.input = np.ctypeslib.as_array(C.cast(self.lib.mgx_bgzf_inflate_batch_input(b), C.POINTER(C.c_uint8)), shape=(in_capacity,))
        io, oo = C.c_void_p(), C.c_void_p()
        native.check(self.lib.mgx_bgzf_inflate_batch_offsets(b, C.byref(io), C.byref(oo)))
        self.in_off = np.ctypeslib.as_array(C.cast(io, C.POINTER(C.c_uint64)), shape=(max_blocks + 1,))
        self.out_off = np.ctypeslib.as_array(C.cast(oo, C.POINTER(C.c_uint64)), shape=(max_blocks + 1,))
        self.n_blocks = 0

    def fill(self, blocks, isizes=None):
        """blocks: whole BGZF members (bytes); the output sizes are their ISIZE fields unless given."""
        at, out = 0, 0
        self.in_off[0] = 0; self.out_off[0] = 0
        for i, blk in enumerate(blocks):
            self.input[at:at + len(blk)] = np.frombuffer(blk, dtype=np.uint8)
            at += len(blk)
            out += isizes[i] if isizes is not None else int.from_bytes(blk[-4:], "little") if len(blk) >= 4 else 0
            self.in_off[i + 1] = at; self.out_off[i + 1] = out
        return len(blocks)

    def submit(self, n_blocks):
        native.check(self.lib.mgx_bgzf_inflate_batch_submit(self.inf.h, self.b, n_blocks))
        self.n_blocks = n_blocks

    def wait(self):
        """(bytes of every block back to back, status word per block, error message or None)."""
        out, st = C.c_void_p(), C.c_void_p()
        rc = self.lib.mgx_bgzf_inflate_batch_wait(self.inf.h, self.b, C.byref(out), C.byref(st))
        err = None
        if rc != 0:
            if rc != -errno.EBADMSG:                             # bad blocks; anything else is a failure
                native.check(rc)
            err = self.lib.mgx_last_error().decode()
        n = self.n_blocks
        total = int(self.out_off[n])
        data = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(max(total, 1),))[:total].tobytes()
        status = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint32)), shape=(max(n, 1),))[:n].copy()
        return data, status, err

    def close(self):
        if self.b:
            self.lib.mgx_bgzf_inflate_batch_destroy(self.inf.h, self.b)
            self.b = None
