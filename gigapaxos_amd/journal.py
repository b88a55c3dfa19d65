"""Journal batches (include/gpx_journal.h): the host side.

`journal_pack` is the host-pointer call: the journal bytes of the ACCEPTs that must be logged - `<be32 len><frame>`
entries in record order, what FileLogger::logBatch builds - cut to what was written, their index rows (the arguments of
LogIndex.add) and the call's `JournalCounts`.  `journal_pack_dev` takes integer device addresses (0 = NULL) and queues
the call on the engine's stream.  `journal_walk` reads such bytes back the way recovery does; it needs no engine.  The
signatures are registered in `_abi._DEV_SIGS` / `_abi._HOST_SIGS` (HIP library only: tests/journal_model.py and
FileLogger::logBatch are the specification of these)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, GpxError, JournalCounts, _i32, _p, _u8, _VP, load_hip  # noqa: F401

JR_COUNT_ONLY = 1  # GPX_JR_COUNT_ONLY
ROW_COLS = (("rec", np.dtype(np.int32)), ("gidx", np.dtype(np.int32)), ("slot", np.dtype(np.int32)),
            ("bnum", np.dtype(np.int32)), ("bcoord", np.dtype(np.int32)), ("off", np.dtype(np.int64)),
            ("len", np.dtype(np.int32)))
ROW_BYTES = sum(dt.itemsize for _, dt in ROW_COLS)  # 32 bytes per index row
COUNTS_BYTES = C.sizeof(JournalCounts)
OUT_ALIGN = 16


def aligned_bytes(n, fill=0) -> np.ndarray:
    """a uint8 array of n bytes whose first byte lies at a multiple of OUT_ALIGN, as `out` must"""
    raw = np.full(int(n) + OUT_ALIGN, fill, np.uint8)
    o = (-raw.ctypes.data) % OUT_ALIGN
    return raw[o:o + int(n)]


def journal_pack(e: Engine, frames, frame_off, gidx, slot, bnum, bcoord, r_flags, status, frame_len=None, rec_frame=None,
                 base_offset=0, flags=0, cap_bytes=None, cap_entries=None, out=None):
    """gpx_journal_pack: (bytes written, the seven row columns in ROW_COLS order cut to n_done, JournalCounts).
    frames: uint8 block; frame_off: int64, n_frames + 1 entries, or n_frames when frame_len is given.  cap_bytes None =
    what every record would need; cap_entries None = n.  `out`: a 16-byte aligned uint8 array of at least cap_bytes to
    write into instead of a fresh one.  With JR_COUNT_ONLY nothing but the counts comes back."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    frame_len = None if frame_len is None else _i32(frame_len)
    n_frames = frame_off.shape[0] - (1 if frame_len is None else 0)
    st = _u8(status)
    n = st.shape[0]
    rf = _u8(r_flags, n)
    cols = [None if c is None else _i32(c, n) for c in (rec_frame, gidx, slot, bnum, bcoord)]
    counts = JournalCounts()
    if int(flags) & JR_COUNT_ONLY:
        outs, rows, cb, ce = None, [None] * len(ROW_COLS), 0, 0
    else:
        ce = n if cap_entries is None else int(cap_entries)
        if cap_bytes is None:  # an upper bound: every record with a frame index in range, whatever its flags
            lens = np.diff(frame_off) if frame_len is None else frame_len.astype(np.int64)
            f = np.arange(n, dtype=np.int64) if cols[0] is None else cols[0].astype(np.int64)
            f = f[(f >= 0) & (f < n_frames)]
            cb = int(np.clip(lens[f], 0, None).sum()) + 4 * int(f.shape[0])
        else:
            cb = int(cap_bytes)
        outs = aligned_bytes(cb) if out is None else out
        if outs.dtype != np.uint8 or outs.shape[0] < cb or outs.ctypes.data % OUT_ALIGN or not outs.flags.c_contiguous:
            raise ValueError("out: a contiguous, 16-byte aligned uint8 array of at least cap_bytes")
        rows = [np.zeros(max(ce, 1), dt) for _, dt in ROW_COLS]
    rc = e.lib.fn["journal_pack"](e.h, n, _p(frames), int(frames.shape[0]), n_frames, _p(frame_off), _p(frame_len),
                                  *[_p(c) for c in cols], _p(rf), _p(st), int(base_offset), int(flags), _p(outs), cb, ce,
                                  *[_p(a) for a in rows], C.byref(counts))
    e.lib.check(rc, "journal_pack")
    if outs is None:
        return None, tuple(rows), counts
    return outs[:int(counts.bytes_done)], tuple(a[:int(counts.n_done)] for a in rows), counts


def _v(p):
    return _VP(int(p)) if p else None


def journal_pack_dev(e: Engine, n, frames_ptr, frames_bytes, n_frames, frame_off_ptr, frame_len_ptr, rec_frame_ptr,
                     col_ptrs, r_flags_ptr, status_ptr, base_offset, flags, out_ptr, cap_bytes, cap_entries, row_ptrs,
                     counts_ptr):
    """gpx_journal_pack_dev: every *_ptr is an integer device address (0 = NULL); col_ptrs = (gidx, slot, bnum, bcoord),
    row_ptrs = the seven row columns in ROW_COLS order, counts_ptr = 32 bytes of device memory.  Asynchronous."""
    e.lib.check(e.lib.fn["journal_pack_dev"](e.h, int(n), _v(frames_ptr), int(frames_bytes), int(n_frames),
                                             _v(frame_off_ptr), _v(frame_len_ptr), _v(rec_frame_ptr),
                                             *[_v(p) for p in col_ptrs], _v(r_flags_ptr), _v(status_ptr), int(base_offset),
                                             int(flags), _v(out_ptr), int(cap_bytes), int(cap_entries),
                                             *[_v(p) for p in row_ptrs], _v(counts_ptr)), "journal_pack_dev")


def journal_walk(buf, base_offset=0, cap=None, lib=None):
    """gpx_journal_walk over a bytes-like: (e_off, e_len of the first min(n_entries, cap) whole entries, n_entries,
    good_bytes).  cap None = as many rows as the buffer could hold."""
    lib = lib or load_hip()
    b = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8)
    cap = b.shape[0] // 4 if cap is None else int(cap)
    e_off, e_len = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
    n, good = C.c_int32(0), C.c_int64(0)
    lib.check(lib.fn["journal_walk"](_p(b) if b.shape[0] else None, int(b.shape[0]), int(base_offset), cap, _p(e_off),
                                     _p(e_len), C.byref(n), C.byref(good)), "journal_walk")
    k = min(int(n.value), cap)
    return e_off[:k], e_len[:k], int(n.value), int(good.value)
