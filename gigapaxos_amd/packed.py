"""Accept-reply votes as packed 8-byte records (include/gpx_packed.h): the host side.

`pack_votes(cols)` runs the library's packer (gpx_votes_pack: pure host code, no GPU needed) over six int32 columns
and returns a `PackedVotes`; `unpack_votes` is its inverse (gpx_votes_unpack).  `Engine.accept_reply_packed_async`
takes a `PackedVotes` in place of the columns: 8 bytes per vote cross the link instead of 24 (16 in the common-ballot
form)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._abi import GpxError, GpxPackedVotes, load_hip

EXC_BIT = 0x80000000
RESERVED_BITS = 0x7F000000
EXC_DIV = 4  # GPX_PACKED_EXC_DIV: the engine takes at most n // 4 exception rows per call


@dataclass
class PackedVotes:
    """A packed batch over host arrays: rec is uint32 [n, 2] (gidx, w), exc int32 [n_exc, 8]."""
    n: int
    n_exc: int
    bnum: int
    bcoord: int
    base_slot: int
    base_cp: int
    base_acceptor: int
    rec: np.ndarray
    exc: np.ndarray
    needed: int = 0  # exception rows the batch needs (gpx_votes_pack's return value; > n_exc: incomplete)

    def struct(self, rec_ptr=None, exc_ptr=None) -> GpxPackedVotes:
        """The C struct: over this batch's own arrays, or with the given (device) addresses."""
        rp = self.rec.ctypes.data if rec_ptr is None else int(rec_ptr)
        ep = self.exc.ctypes.data if exc_ptr is None else int(exc_ptr)
        return GpxPackedVotes(self.n, self.n_exc, self.bnum, self.bcoord, self.base_slot, self.base_cp,
                              self.base_acceptor, 0, rp or None, ep or None)

    @property
    def nbytes(self) -> int:
        """What crosses the link for this batch."""
        return 8 * self.n + 32 * self.n_exc


def pack_votes(cols, engine=None, lib=None, exc_cap=None, rec_out=None, exc_out=None) -> PackedVotes:
    """gpx_votes_pack over (gidx, bnum, bcoord, slot, acceptor, max_cp).  The record and exception arrays come from
    `engine.host_alloc` when an engine is given (the DMA engines reach them at the link's full rate), else plain numpy;
    `rec_out` / `exc_out` reuse arrays of the caller.  exc_cap defaults to n // 4, the most the engine takes; a batch
    that needs more comes back with needed > n_exc (submit its plain columns instead)."""
    lib = lib or (engine.lib if engine is not None else load_hip())
    cols = [np.ascontiguousarray(c, dtype=np.int32) for c in cols]
    n = int(cols[0].shape[0])
    if len(cols) != 6 or any(c.shape != (n,) for c in cols):
        raise ValueError("six int32 columns of one length")
    if exc_cap is None:
        exc_cap = n // EXC_DIV if exc_out is None else exc_out.size // 8
    mk = engine.host_alloc if engine is not None else np.zeros
    rec = mk(2 * max(n, 1), np.uint32) if rec_out is None else rec_out
    exc = mk(8 * max(exc_cap, 1), np.int32) if exc_out is None else exc_out
    if rec.dtype != np.uint32 or rec.size < 2 * n or exc.dtype != np.int32 or exc.size < 8 * exc_cap:
        raise ValueError("rec_out: uint32 [2 n], exc_out: int32 [8 exc_cap]")
    pv = GpxPackedVotes()
    need = lib.fn["votes_pack"](n, *[c.ctypes.data_as(C.c_void_p) for c in cols], rec.ctypes.data_as(C.c_void_p),
                                exc.ctypes.data_as(C.c_void_p), int(exc_cap), C.byref(pv))
    if need < 0:
        raise GpxError(f"gpx_votes_pack failed rc={need}")
    return PackedVotes(pv.n, pv.n_exc, pv.bnum, pv.bcoord, pv.base_slot, pv.base_cp, pv.base_acceptor,
                       rec.reshape(-1)[:2 * max(n, 1)].reshape(-1, 2)[:n], exc.reshape(-1)[:8 * pv.n_exc].reshape(-1, 8),
                       int(need))


def unpack_votes(packed: PackedVotes, lib=None):
    """gpx_votes_unpack: the six int32 columns a packed batch stands for, in record order."""
    lib = lib or load_hip()
    cols = [np.zeros(packed.n, np.int32) for _ in range(6)]
    pv = packed.struct()
    rc = lib.fn["votes_unpack"](C.byref(pv), *[c.ctypes.data_as(C.c_void_p) for c in cols])
    if rc < 0:
        raise GpxError(f"gpx_votes_unpack failed rc={rc}")
    return tuple(cols)
