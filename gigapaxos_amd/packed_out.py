"""Proposals and decisions as packed records in one buffer (include/gpx_packed_out.h): the host side.

`pack_decisions(cols)` / `pack_proposals(cols)` run the library's packers (pure host code, no GPU needed) over the
plain output columns and return a `PackedOut`; `unpack_decisions` / `unpack_proposals` are their inverses, for either
form.  `Engine.propose_packed_out_async` and `Engine.accept_reply_packed_io_async` hand such a buffer back in place of
the columns: 4 bytes per proposal and 8 per decision cross the link in the steady state instead of 17 and 21."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import GpxError, GpxPackedOutHdr, load_hip

RECORDS, COLUMNS = 1, 2
DECISIONS, PROPOSALS = 1, 2
EXC_BIT = 0x80000000
EXC_DIV = 4  # RECORDS carries at most n // 4 rows; a call that needs more comes back in the COLUMNS form


def _r32(x: int) -> int:
    return (int(x) + 31) & ~31


def packed_out_bytes(cap: int) -> int:
    """GPX_PACKED_OUT_BYTES(cap): what a buffer for up to `cap` entries must hold (either kind, either form)."""
    return 32 + 5 * _r32(4 * cap) + _r32(cap)


def _buf(buf) -> np.ndarray:
    a = np.asarray(buf)
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("a packed output is a contiguous uint8 array")
    return a


class PackedOut:
    """A view of a packed output buffer: the header's fields, `nbytes` = the bytes the buffer uses (what crossed the
    link), `raw` = those bytes.  `needed` is the packer's return value when the view comes from pack_*."""

    def __init__(self, buf, lib=None, needed=None):
        self.buf = _buf(buf)
        if self.buf.nbytes < 32:
            raise GpxError("a packed output starts with a 32-byte header")
        h = GpxPackedOutHdr.from_buffer_copy(self.buf[:32].tobytes())
        self.form, self.kind, self.n, self.n_exc = h.form, h.kind, h.n, h.n_exc
        self.bnum, self.bcoord, self.base_slot, self.base_cp = h.bnum, h.bcoord, h.base_slot, h.base_cp
        self.needed = needed
        lib = lib or load_hip()
        size = int(lib.fn["packed_out_size"](self.buf.ctypes.data_as(C.c_void_p)))
        if size < 0 or size > self.buf.nbytes:
            raise GpxError(f"not a packed output (gpx_packed_out_size = {size} for {self.buf.nbytes} bytes)")
        self.nbytes = size

    @property
    def raw(self) -> np.ndarray:
        return self.buf[:self.nbytes]

    def header(self) -> dict:
        return dict(form=self.form, kind=self.kind, n=self.n, n_exc=self.n_exc, bnum=self.bnum, bcoord=self.bcoord,
                    base_slot=self.base_slot, base_cp=self.base_cp)

    def unpack(self, lib=None):
        return (unpack_decisions if self.kind == DECISIONS else unpack_proposals)(self.buf, lib=lib)


def _pack(name, cols, byte_col, lib, out):
    lib = lib or load_hip()
    cols = [np.ascontiguousarray(c, dtype=np.int32) for c in cols]
    b = np.ascontiguousarray(byte_col, dtype=np.uint8)
    n = int(b.shape[0])
    if any(c.shape != (n,) for c in cols):
        raise ValueError("columns of one length")
    out = np.zeros(packed_out_bytes(n), np.uint8) if out is None else _buf(out)
    need = lib.fn[name](n, *[c.ctypes.data_as(C.c_void_p) for c in cols], b.ctypes.data_as(C.c_void_p),
                        out.ctypes.data_as(C.c_void_p), out.nbytes)
    if need < 0:
        raise GpxError(f"gpx_{name} failed rc={need}")
    return PackedOut(out, lib=lib, needed=int(need))


def pack_decisions(cols, lib=None, out=None) -> PackedOut:
    """gpx_decisions_pack over (d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, d_kind)."""
    if len(cols) != 6:
        raise ValueError("five int32 columns and the d_kind bytes")
    return _pack("decisions_pack", cols[:5], cols[5], lib, out)


def pack_proposals(cols, lib=None, out=None) -> PackedOut:
    """gpx_proposals_pack over (slot, bnum, bcoord, median_cp, status)."""
    if len(cols) != 5:
        raise ValueError("four int32 columns and the status bytes")
    return _pack("proposals_pack", cols[:4], cols[4], lib, out)


def _unpack(name, ncols, buf, lib, nbytes):
    lib = lib or load_hip()
    buf = _buf(buf)
    nbytes = buf.nbytes if nbytes is None else int(nbytes)
    if nbytes > buf.nbytes:
        raise ValueError("nbytes beyond the array")
    cap = 0
    if nbytes >= 32:
        cap = int(buf[8:12].view(np.int32)[0])
    cap = max(0, min(cap, nbytes))  # an entry takes a byte at the least: a header that promises more is refused below
    cols = [np.zeros(cap, np.int32) for _ in range(ncols)]
    b = np.zeros(cap, np.uint8)
    n = C.c_int32(0)
    rc = lib.fn[name](buf.ctypes.data_as(C.c_void_p), nbytes, cap, *[c.ctypes.data_as(C.c_void_p) for c in cols],
                      b.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc < 0:
        raise GpxError(f"gpx_{name} failed rc={rc}")
    return tuple(c[:n.value] for c in cols) + (b[:n.value],)


def unpack_decisions(buf, lib=None, nbytes=None):
    """gpx_decisions_unpack: (d_gidx, d_slot, d_bnum, d_bcoord, d_median_cp, d_kind) of a buffer in either form."""
    return _unpack("decisions_unpack", 5, buf, lib, nbytes)


def unpack_proposals(buf, lib=None, nbytes=None):
    """gpx_proposals_unpack: (slot, bnum, bcoord, median_cp, status) of a buffer in either form."""
    return _unpack("proposals_unpack", 4, buf, lib, nbytes)
