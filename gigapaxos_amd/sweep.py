"""The deactivation sweep (include/gpx_sweep.h): the host side.

`pause_sweep` is the host-pointer call: (gidx, age, rows) of the groups the call handed back - and, unless it only
peeked, paused - cut to what was written, plus the call's `SweepCounts`.  `pause_sweep_dev` takes integer device
addresses (0 = NULL) and queues the sweep on the engine's stream.  The signatures are registered in `_abi._DEV_SIGS`
(HIP library only: the CPU oracle's group_retire, group_snapshot and group_dump are the specification of these)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, HRI_DTYPE, SweepCounts, _i32, _p, _VP  # noqa: F401  (SweepCounts: part of this module's interface)

SWEEP_PEEK, SWEEP_HOLD = 1, 2  # GPX_SWEEP_PEEK, GPX_SWEEP_HOLD
SWEEP_COLS = (("gidx", np.dtype(np.int32)), ("age", np.dtype(np.uint8)), ("rows", HRI_DTYPE))
HIT_BYTES = sum(dt.itemsize for _, dt in SWEEP_COLS)  # 105 bytes per paused group cross the link, plus the counts
COUNTS_BYTES = C.sizeof(SweepCounts)


def pause_sweep(e: Engine, gidx=None, min_age=1, flags=0, cap=None, n=None, out=None):
    """gpx_pause_sweep: ((gidx, age, rows) of the first min(n_hits, cap) hits, SweepCounts).  gidx None = groups
    0 .. n-1 (n None: the whole table); cap None = n.  `out`: three arrays of at least cap entries (int32, uint8,
    HRI_DTYPE) to write into instead of fresh ones; cap == 0 without `out` passes null columns and only counts."""
    if gidx is None:
        n, g = (int(e.cfg.max_groups) if n is None else int(n)), None
    else:
        g = _i32(gidx)
        n = g.shape[0]
    cap = n if cap is None else int(cap)
    if cap == 0 and out is None:
        outs = [None] * 3
    elif out is None:
        outs = [np.zeros(cap, dt) for _, dt in SWEEP_COLS]
    else:
        outs = list(out)
        if len(outs) != 3 or any(a.dtype != dt or a.shape[0] < cap or not a.flags.c_contiguous
                                 for a, (_, dt) in zip(outs, SWEEP_COLS)):
            raise ValueError("out: one contiguous array of the column's dtype and at least cap entries per column")
    counts = SweepCounts()
    rc = e.lib.fn["pause_sweep"](e.h, n, _p(g), int(min_age), int(flags), cap, *[_p(a) for a in outs], C.byref(counts))
    e.lib.check(rc, "pause_sweep")
    k = max(0, min(int(counts.n_hits), cap))
    return tuple(None if a is None else a[:k] for a in outs), counts


def _v(p):
    return _VP(int(p)) if p else None


def pause_sweep_dev(e: Engine, n, gidx_ptr, min_age, flags, cap, out_ptrs, counts_ptr):
    """gpx_pause_sweep_dev: gidx_ptr, the three out_ptrs (o_gidx, o_age, o_rows) and counts_ptr are integer device
    addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["pause_sweep_dev"](e.h, int(n), _v(gidx_ptr), int(min_age), int(flags), int(cap),
                                            *[_v(p) for p in out_ptrs], _v(counts_ptr)), "pause_sweep_dev")
