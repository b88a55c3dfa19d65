"""Journal compaction (include/gpx_journal_gc.h): the host side.

`journal_gc` is the host-pointer call: of the logged ACCEPTs the index rows name, the entries garbage collection still
needs - byte for byte as they stand in `data`, contiguous, in row order - their new index rows, the per-row verdicts
and the call's `JournalGcCounts`, from which the caller reads compactLogfile's three outcomes (`outcome`).
`journal_gc_dev` takes integer device addresses (0 = NULL) and queues the call on the engine's stream.  The signatures
are registered in `_abi._DEV_SIGS` (HIP library only: tests/journal_gc_model.py is the specification)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, GpxError, JournalGcCounts, _i32, _p, _VP  # noqa: F401
from .journal import OUT_ALIGN, aligned_bytes

JG_COUNT_ONLY, JG_SKIP_UNCHANGED = 1, 2                  # GPX_JG_COUNT_ONLY, GPX_JG_SKIP_UNCHANGED
JG_DROP, JG_KEEP, JG_KEEP_UNJUDGED, JG_BAD = 0, 1, 2, 3  # GPX_JG_*: the verdicts
ROW_COLS = (("src", np.dtype(np.int32)), ("gidx", np.dtype(np.int32)), ("slot", np.dtype(np.int32)),
            ("bnum", np.dtype(np.int32)), ("bcoord", np.dtype(np.int32)), ("off", np.dtype(np.int64)),
            ("len", np.dtype(np.int32)))
COUNTS_BYTES = C.sizeof(JournalGcCounts)
DELETE, LEAVE, REPLACE = "delete", "leave", "replace"


def outcome(counts) -> str:
    """compactLogfile's three outcomes (SQLPaxosLogger.java:3420-3436) from the counts of a call that was not cut; a
    caller must not act on REPLACE when counts.n_bad > 0"""
    if counts.n_keep == 0:
        return DELETE
    return LEAVE if counts.unchanged else REPLACE


def journal_gc(e: Engine, data, e_gidx, e_slot, e_off, e_len, e_bnum=None, e_bcoord=None, cp_slot=None, in_base=0,
               out_base=0, flags=0, cap_bytes=None, cap_entries=None, in_bytes=None, want_verdict=True):
    """gpx_journal_gc: (bytes written, the seven k_* columns in ROW_COLS order cut to n_done - bnum / bcoord None where
    e_bnum / e_bcoord are -, verdicts, JournalGcCounts).  data: a uint8 block (copied to a 16-byte aligned one whose
    size is a multiple of 16 unless it already is) or None with JG_COUNT_ONLY; cap_bytes None = the sum of 4 + len over
    the rows with a length in range; cap_entries None = n."""
    e_len = _i32(e_len)
    n = e_len.shape[0]
    e_gidx, e_slot = _i32(e_gidx, n), _i32(e_slot, n)
    e_off = np.ascontiguousarray(e_off, dtype=np.int64)
    if e_off.shape[0] != n:
        raise ValueError("column length mismatch")
    opt = [None if c is None else _i32(c, n) for c in (e_bnum, e_bcoord, cp_slot)]
    if data is None:
        blk, nb = None, int(in_bytes or 0)
    else:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        nb = data.shape[0] if in_bytes is None else int(in_bytes)
        if data.ctypes.data % OUT_ALIGN or data.shape[0] % 16:
            blk = aligned_bytes((data.shape[0] + 15) // 16 * 16)
            blk[:data.shape[0]] = data
        else:
            blk = data
    counts = JournalGcCounts()
    verdict = np.full(max(n, 1), 0xFF, np.uint8) if want_verdict else None
    if int(flags) & JG_COUNT_ONLY:
        outs, rows, cb, ce = None, [None] * len(ROW_COLS), 0, 0
    else:
        ce = n if cap_entries is None else int(cap_entries)
        if cap_bytes is None:
            ln = e_len.astype(np.int64)
            cb = int((ln[(ln >= 0) & (ln <= nb)] + 4).sum())
        else:
            cb = int(cap_bytes)
        outs = aligned_bytes(cb)
        rows = [np.zeros(max(ce, 1), dt) for _, dt in ROW_COLS]
        if opt[0] is None:
            rows[3] = None
        if opt[1] is None:
            rows[4] = None
    rc = e.lib.fn["journal_gc"](e.h, n, _p(blk), nb, int(in_base), _p(e_gidx), _p(e_slot), _p(e_off), _p(e_len),
                                *[_p(c) for c in opt], int(out_base), int(flags), _p(outs), cb, ce, _p(verdict),
                                *[_p(a) for a in rows], C.byref(counts))
    e.lib.check(rc, "journal_gc")
    v = None if verdict is None else verdict[:n]
    if outs is None:
        return None, tuple(rows), v, counts
    return (outs[:int(counts.bytes_done)], tuple(None if a is None else a[:int(counts.n_done)] for a in rows), v, counts)


def _v(p):
    return _VP(int(p)) if p else None


def journal_gc_dev(e: Engine, n, in_ptr, in_bytes, in_base, col_ptrs, out_base, flags, out_ptr, cap_bytes, cap_entries,
                   verdict_ptr, row_ptrs, counts_ptr):
    """gpx_journal_gc_dev: every *_ptr is an integer device address (0 = NULL); col_ptrs = (e_gidx, e_slot, e_off, e_len,
    e_bnum, e_bcoord, cp_slot), row_ptrs = the seven k_* columns in ROW_COLS order, counts_ptr = 64 bytes of device
    memory.  Asynchronous."""
    e.lib.check(e.lib.fn["journal_gc_dev"](e.h, int(n), _v(in_ptr), int(in_bytes), int(in_base),
                                           *[_v(p) for p in col_ptrs], int(out_base), int(flags), _v(out_ptr),
                                           int(cap_bytes), int(cap_entries), _v(verdict_ptr), *[_v(p) for p in row_ptrs],
                                           _v(counts_ptr)), "journal_gc_dev")
