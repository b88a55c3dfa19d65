"""Checkpoint transfer (include/gpx_checkpoint.h): the host side.

`checkpoint_batch` is the host-pointer call: one StatePacket(slotNumber = cp_slot[i]) per record for group gidx[i]; it
returns the dense columns (from, to, flags, status), the execution runs cut to what was written, and the call's
`CpCounts`.  `checkpoint_batch_dev` takes integer device addresses (0 = NULL) and queues the call on the engine's
stream.  The signatures are registered in `_abi._DEV_SIGS` (HIP library only).

The reference restores the app state BEFORE it moves the acceptor and does nothing if the restore fails
(PISM:1853-1858): peek (`CP_PEEK`), restore the app state of the records flagged `CP_ADOPT`, then apply the records whose
restore succeeded."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import CpCounts, Engine, _i32, _p, _VP  # noqa: F401  (CpCounts: part of this module's interface)

CP_PEEK = 1               # GPX_CP_PEEK (call flag)
CP_ADOPT, CP_MOVED = 1, 2  # GPX_CP_ADOPT, GPX_CP_MOVED (o_flags)
COUNTS_BYTES = C.sizeof(CpCounts)
IN_BYTES, OUT_BYTES, RUN_BYTES = 8, 10, 12  # what crosses the link per record (in, out) and per run


def checkpoint_batch(e: Engine, gidx, cp_slot, flags=0):
    """gpx_checkpoint_batch: ((o_from, o_to, o_flags, status), runs [n_runs, 3] of (gidx, first, count), CpCounts)."""
    g, cp = _i32(gidx), _i32(cp_slot)
    n = g.shape[0]
    if cp.shape[0] != n:
        raise ValueError("gidx and cp_slot: one entry per record each")
    o_from, o_to = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    o_flags, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    peek = bool(int(flags) & CP_PEEK)
    xs = [None] * 3 if peek else [np.zeros(max(n, 1), np.int32) for _ in range(3)]
    counts = CpCounts()
    # a column of no entries still needs an address: the call refuses null columns before it looks at n
    gp, cpp = (np.zeros(1, np.int32), np.zeros(1, np.int32)) if n == 0 else (g, cp)
    rc = e.lib.fn["checkpoint_batch"](e.h, n, _p(gp), _p(cpp), int(flags), _p(o_from), _p(o_to), _p(o_flags), _p(status),
                                      *[_p(a) for a in xs], C.byref(counts))
    e.lib.check(rc, "checkpoint_batch")
    k = 0 if peek else max(0, min(int(counts.n_runs), n))
    runs = np.zeros((k, 3), np.int32) if peek else np.stack([a[:k] for a in xs], axis=1)
    return (o_from[:n], o_to[:n], o_flags[:n], status[:n]), runs, counts


def _v(p):
    return _VP(int(p)) if p else None


def checkpoint_batch_dev(e: Engine, n, gidx_ptr, cp_slot_ptr, flags, dense_ptrs, run_ptrs, counts_ptr):
    """gpx_checkpoint_batch_dev: gidx_ptr, cp_slot_ptr, the four dense_ptrs (o_from, o_to, o_flags, status), the three
    run_ptrs (x_gidx, x_first, x_count) and counts_ptr are integer device addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["checkpoint_batch_dev"](e.h, int(n), _v(gidx_ptr), _v(cp_slot_ptr), int(flags),
                                                 *[_v(p) for p in dense_ptrs], *[_v(p) for p in run_ptrs],
                                                 _v(counts_ptr)), "checkpoint_batch_dev")
