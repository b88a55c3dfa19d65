"""Retransmission timers on the device (include/gpx_timers.h): the host side.

`retransmit_sweep` is the host-pointer call: the ten columns of the due ACCEPTs and PREPAREs - what gpx_poke_scan
writes for their groups, plus the retransmission count after this one and the wait - cut to what was written, and the
call's `RtxCounts`.  `retransmit_sweep_dev` takes integer device addresses (0 = NULL) and queues the sweep on the
engine's stream.  `backoff_table` is the reference's back-off as the integer table the device compares with.  The
signatures are registered in `_abi._DEV_SIGS` (HIP library only: the CPU oracle's poke_scan and tests/timers_model.py
are the specification of these)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, GpxError, RtxCfg, RtxCounts, RTX_MAX_STEPS, _i32, _p, _VP, load_hip  # noqa: F401

RTX_PEEK = 1  # GPX_RTX_PEEK
RTX_COLS = (("gidx", np.dtype(np.int32)), ("poke", np.dtype(np.uint8)), ("slot", np.dtype(np.int32)),
            ("bnum", np.dtype(np.int32)), ("bcoord", np.dtype(np.int32)), ("median_cp", np.dtype(np.int32)),
            ("flags", np.dtype(np.uint8)), ("heard", np.dtype(np.uint32)), ("count", np.dtype(np.uint8)),
            ("waited", np.dtype(np.int32)))
HIT_BYTES = sum(dt.itemsize for _, dt in RTX_COLS)  # 31 bytes per due entry cross the link, plus the counts
COUNTS_BYTES = C.sizeof(RtxCounts)


def backoff_table(timeout_ms, factor=1.5, n_steps=RTX_MAX_STEPS, lib=None) -> np.ndarray:
    """gpx_rtx_backoff_table: out[c] = min(floor(timeout_ms * factor**c), INT32_MAX), c < n_steps."""
    lib = lib or load_hip()
    out = np.zeros(max(int(n_steps), 1), np.int32)
    lib.check(lib.fn["rtx_backoff_table"](int(timeout_ms), float(factor), int(n_steps), _p(out)), "rtx_backoff_table")
    return out[:int(n_steps)]


def make_cfg(accept_ms, prepare_ms=None) -> RtxCfg:
    """An RtxCfg from one or two threshold tables of equal length (prepare_ms None: the ACCEPT table for both kinds)."""
    a = [int(x) for x in accept_ms]
    p = a if prepare_ms is None else [int(x) for x in prepare_ms]
    if len(a) != len(p) or not 1 <= len(a) <= RTX_MAX_STEPS:
        raise ValueError("1 .. %d thresholds per kind, as many for PREPARE as for ACCEPT" % RTX_MAX_STEPS)
    cfg = RtxCfg()
    cfg.n_steps = len(a)
    cfg.accept_ms[:len(a)] = a
    cfg.prepare_ms[:len(p)] = p
    return cfg


def retransmit_sweep(e: Engine, now_ms, cfg: RtxCfg, gidx=None, flags=0, cap=None, n=None, out=None):
    """gpx_retransmit_sweep: (the ten columns of the first min(n_hits, cap) hits in RTX_COLS order, RtxCounts).  gidx
    None = groups 0 .. n-1 (n None: the whole table); cap None = n.  now_ms: any integer, taken modulo 2^32.  `out`: ten
    arrays of at least cap entries to write into instead of fresh ones; cap == 0 without `out` passes null columns and
    only counts."""
    if gidx is None:
        n, g = (int(e.cfg.max_groups) if n is None else int(n)), None
    else:
        g = _i32(gidx)
        n = g.shape[0]
    cap = n if cap is None else int(cap)
    if cap == 0 and out is None:
        outs = [None] * len(RTX_COLS)
    elif out is None:
        outs = [np.zeros(cap, dt) for _, dt in RTX_COLS]
    else:
        outs = list(out)
        if len(outs) != len(RTX_COLS) or any(a.dtype != dt or a.shape[0] < cap or not a.flags.c_contiguous
                                             for a, (_, dt) in zip(outs, RTX_COLS)):
            raise ValueError("out: one contiguous array of the column's dtype and at least cap entries per column")
    counts = RtxCounts()
    rc = e.lib.fn["retransmit_sweep"](e.h, n, _p(g), wrap_ms(now_ms), C.byref(cfg), int(flags), cap,
                                      *[_p(a) for a in outs], C.byref(counts))
    e.lib.check(rc, "retransmit_sweep")
    k = max(0, min(int(counts.n_hits), cap))
    return tuple(None if a is None else a[:k] for a in outs), counts


def wrap_ms(now_ms) -> int:
    """a clock value as the int32 the call takes: modulo 2^32, two's complement"""
    return ((int(now_ms) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _v(p):
    return _VP(int(p)) if p else None


def retransmit_sweep_dev(e: Engine, n, gidx_ptr, now_ms, cfg: RtxCfg, flags, cap, out_ptrs, counts_ptr):
    """gpx_retransmit_sweep_dev: gidx_ptr, the ten out_ptrs (RTX_COLS order) and counts_ptr are integer device
    addresses (0 = NULL); cfg is host memory.  Asynchronous."""
    e.lib.check(e.lib.fn["retransmit_sweep_dev"](e.h, int(n), _v(gidx_ptr), wrap_ms(now_ms), C.byref(cfg), int(flags),
                                                 int(cap), *[_v(p) for p in out_ptrs], _v(counts_ptr)),
                "retransmit_sweep_dev")
