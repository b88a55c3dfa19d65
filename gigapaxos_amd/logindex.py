"""The log index on the device (include/gpx_logindex.h): the host side.

`open` allocates the index; `add`, `set_gc`, `lookup`, `file_rows`, `relocate`, `files` and `compact` are the
host-pointer calls on numpy columns; the functions that end in `_dev` take integer device addresses (0 = NULL) and queue
the call on the engine's stream.  The signatures are registered in `_abi._DEV_SIGS` (HIP library only:
tests/logindex_model.py is the specification)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, GpxError, LogIndexCounts, _i32, _p, _u8, _VP  # noqa: F401

LI_ADDED, LI_STALE, LI_NOGROUP, LI_FULL, LI_REPEAT = 0, 1, 2, 3, 4  # GPX_LI_*: the status bytes
LI_RESET = 1                                                       # GPX_LI_RESET
LI_MAX_FILES = 4096                                                # GPX_LI_MAX_FILES
COUNTS_BYTES = C.sizeof(LogIndexCounts)
# lookup's output columns, file_rows' output columns
LOOKUP_COLS = (("rec", np.int32), ("row", np.int32), ("slot", np.int32), ("bnum", np.int32), ("bcoord", np.int32),
               ("file", np.int32), ("off", np.int64), ("len", np.int32))
FILE_ROWS_COLS = (("row", np.int32), ("gidx", np.int32), ("slot", np.int32), ("bnum", np.int32), ("bcoord", np.int32),
                  ("off", np.int64), ("len", np.int32), ("gc", np.int32))


def _i64(a, n):
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.shape[0] != n:
        raise ValueError("column length mismatch")
    return a


def _n_dev(v):
    return None if v is None else np.array([int(v)], np.int32)


def open(e: Engine, cap_rows: int) -> None:
    """gpx_logindex_open: a table of cap_rows rows; once per engine"""
    e.lib.check(e.lib.fn["logindex_open"](e.h, int(cap_rows)), "logindex_open")


def add(e: Engine, e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len, file, n_dev=None):
    """gpx_logindex_add -> (status bytes of the records taken, LogIndexCounts)"""
    e_gidx = _i32(e_gidx)
    n = e_gidx.shape[0]
    cols = [e_gidx, _i32(e_slot, n), _i32(e_bnum, n), _i32(e_bcoord, n), _i64(e_off, n), _i32(e_len, n)]
    nd = _n_dev(n_dev)
    status = np.full(max(n, 1), 0xFF, np.uint8)
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_add"](e.h, n, _p(nd), *[_p(c) for c in cols], int(file), _p(status), C.byref(counts))
    e.lib.check(rc, "logindex_add")
    m = n if nd is None else min(n, max(int(nd[0]), 0))
    return status[:m], counts


def set_gc(e: Engine, gidx, gc_slot=None, flags=0):
    """gpx_logindex_set_gc -> (status bytes, LogIndexCounts); gc_slot None only with LI_RESET"""
    gidx = _i32(gidx)
    n = gidx.shape[0]
    gc_slot = None if gc_slot is None else _i32(gc_slot, n)
    status = np.full(max(n, 1), 0xFF, np.uint8)
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_set_gc"](e.h, n, _p(gidx), _p(gc_slot), int(flags), _p(status), C.byref(counts))
    e.lib.check(rc, "logindex_set_gc")
    return status[:n], counts


def lookup(e: Engine, gidx, min_slot, max_slot=None, has_max=None, cap=0):
    """gpx_logindex_lookup -> (dict of LOOKUP_COLS cut to n_done, status bytes, LogIndexCounts)"""
    gidx = _i32(gidx)
    n = gidx.shape[0]
    min_slot = _i32(min_slot, n)
    max_slot = None if max_slot is None else _i32(max_slot, n)
    has_max = _u8(has_max, n)
    cap = int(cap)
    outs = [np.zeros(cap, dt) if cap > 0 else None for _, dt in LOOKUP_COLS]
    status = np.full(max(n, 1), 0xFF, np.uint8)
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_lookup"](e.h, n, _p(gidx), _p(min_slot), _p(max_slot), _p(has_max), cap,
                                     *[_p(a) for a in outs], _p(status), C.byref(counts))
    e.lib.check(rc, "logindex_lookup")
    k = int(counts.n_done)
    return ({name: (np.zeros(0, dt) if a is None else a[:k]) for (name, dt), a in zip(LOOKUP_COLS, outs)}, status[:n],
            counts)


def file_rows(e: Engine, file, cap):
    """gpx_logindex_file_rows -> (dict of FILE_ROWS_COLS cut to n_done, LogIndexCounts)"""
    cap = int(cap)
    outs = [np.zeros(cap, dt) if cap > 0 else None for _, dt in FILE_ROWS_COLS]
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_file_rows"](e.h, int(file), cap, *[_p(a) for a in outs], C.byref(counts))
    e.lib.check(rc, "logindex_file_rows")
    k = int(counts.n_done)
    return {name: (np.zeros(0, dt) if a is None else a[:k]) for (name, dt), a in zip(FILE_ROWS_COLS, outs)}, counts


def relocate(e: Engine, generation, o_row, k_src, new_file, k_off, k_len, n_dev=None):
    """gpx_logindex_relocate -> LogIndexCounts; k_src None: row j of o_row"""
    o_row = _i32(o_row)
    n = o_row.shape[0]
    k_src = None if k_src is None else _i32(k_src, n)
    nd = _n_dev(n_dev)
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_relocate"](e.h, n, _p(nd), int(generation), _p(o_row), _p(k_src), int(new_file),
                                       _p(_i64(k_off, n)), _p(_i32(k_len, n)), C.byref(counts))
    e.lib.check(rc, "logindex_relocate")
    return counts


def files(e: Engine, file_base, n_files):
    """gpx_logindex_files -> (alive rows per file, groups per min file, the smallest min file or -1, LogIndexCounts)"""
    n_files = int(n_files)
    rows, groups = np.zeros(max(n_files, 1), np.int32), np.zeros(max(n_files, 1), np.int32)
    lo = np.zeros(1, np.int32)
    counts = LogIndexCounts()
    rc = e.lib.fn["logindex_files"](e.h, int(file_base), n_files, _p(rows), _p(groups), _p(lo), C.byref(counts))
    e.lib.check(rc, "logindex_files")
    return rows[:n_files], groups[:n_files], int(lo[0]), counts


def compact(e: Engine):
    """gpx_logindex_compact -> LogIndexCounts"""
    counts = LogIndexCounts()
    e.lib.check(e.lib.fn["logindex_compact"](e.h, C.byref(counts)), "logindex_compact")
    return counts


def _v(p):
    return _VP(int(p)) if p else None


def add_dev(e: Engine, n, n_dev_ptr, col_ptrs, file, status_ptr, counts_ptr):
    """gpx_logindex_add_dev: col_ptrs = (e_gidx, e_slot, e_bnum, e_bcoord, e_off, e_len).  Asynchronous, as every _dev."""
    e.lib.check(e.lib.fn["logindex_add_dev"](e.h, int(n), _v(n_dev_ptr), *[_v(p) for p in col_ptrs], int(file),
                                             _v(status_ptr), _v(counts_ptr)), "logindex_add_dev")


def set_gc_dev(e: Engine, n, gidx_ptr, gc_slot_ptr, flags, status_ptr, counts_ptr):
    e.lib.check(e.lib.fn["logindex_set_gc_dev"](e.h, int(n), _v(gidx_ptr), _v(gc_slot_ptr), int(flags), _v(status_ptr),
                                                _v(counts_ptr)), "logindex_set_gc_dev")


def lookup_dev(e: Engine, n, gidx_ptr, min_ptr, max_ptr, has_max_ptr, cap, out_ptrs, status_ptr, counts_ptr):
    """out_ptrs: the eight columns in LOOKUP_COLS order"""
    e.lib.check(e.lib.fn["logindex_lookup_dev"](e.h, int(n), _v(gidx_ptr), _v(min_ptr), _v(max_ptr), _v(has_max_ptr),
                                                int(cap), *[_v(p) for p in out_ptrs], _v(status_ptr), _v(counts_ptr)),
                "logindex_lookup_dev")


def file_rows_dev(e: Engine, file, cap, out_ptrs, counts_ptr):
    """out_ptrs: the eight columns in FILE_ROWS_COLS order"""
    e.lib.check(e.lib.fn["logindex_file_rows_dev"](e.h, int(file), int(cap), *[_v(p) for p in out_ptrs], _v(counts_ptr)),
                "logindex_file_rows_dev")


def relocate_dev(e: Engine, n, n_dev_ptr, generation, o_row_ptr, k_src_ptr, new_file, k_off_ptr, k_len_ptr, counts_ptr):
    e.lib.check(e.lib.fn["logindex_relocate_dev"](e.h, int(n), _v(n_dev_ptr), int(generation), _v(o_row_ptr),
                                                  _v(k_src_ptr), int(new_file), _v(k_off_ptr), _v(k_len_ptr),
                                                  _v(counts_ptr)), "logindex_relocate_dev")


def files_dev(e: Engine, file_base, n_files, o_rows_ptr, o_groups_ptr, o_min_file_ptr, counts_ptr):
    e.lib.check(e.lib.fn["logindex_files_dev"](e.h, int(file_base), int(n_files), _v(o_rows_ptr), _v(o_groups_ptr),
                                               _v(o_min_file_ptr), _v(counts_ptr)), "logindex_files_dev")


def compact_dev(e: Engine, counts_ptr):
    e.lib.check(e.lib.fn["logindex_compact_dev"](e.h, _v(counts_ptr)), "logindex_compact_dev")
