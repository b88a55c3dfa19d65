"""Table scans that return only their hits (include/gpx_scan.h): the host side.

`election_scan_hits`, `poke_scan_hits` and `gap_scan_hits` are the host-pointer calls: numpy arrays out, cut to the hits
the call wrote, plus the call's `ScanCounts`.  Their `_dev` forms take integer device addresses (0 = NULL) and queue the
scan on the engine's stream; `election_begin_hits_dev` runs gpx_election_begin over a scan's output with the count read
on the device.  The signatures are registered in `_abi._DEV_SIGS` (HIP library only: the CPU oracle has the dense scans,
which are the specification of these)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, ScanCounts, _i32, _p, _VP  # noqa: F401  (ScanCounts: part of this module's interface)

SCAN_TILE = 1024  # GPX_SCAN_TILE
GAP_HIT_SYNC, GAP_HIT_MISSING, GAP_HIT_AHEAD = 1, 2, 4
SYNC_DEFAULT, SYNC_TO_PAUSE, SYNC_FORCE = 0, 1, 2

# the compact columns of each scan, in argument order: (name, dtype); bytes per hit = 13, 26, 21
ELECTION_COLS = (("gidx", np.int32), ("run", np.uint8), ("bnum", np.int32), ("first", np.int32))
POKE_COLS = (("gidx", np.int32), ("poke", np.uint8), ("slot", np.int32), ("bnum", np.int32), ("bcoord", np.int32),
             ("median_cp", np.int32), ("flags", np.uint8), ("heard", np.uint32))
GAP_COLS = (("gidx", np.int32), ("first", np.int32), ("max_committed", np.int32), ("missing", np.uint64),
            ("sync", np.uint8))
HIT_BYTES = {"election": 13, "poke": 26, "gap": 21}
COUNTS_BYTES = C.sizeof(ScanCounts)


def _scanned(e: Engine, gidx, n):
    if gidx is None:
        return (int(e.cfg.max_groups) if n is None else int(n)), None
    g = _i32(gidx)
    return g.shape[0], g


def _outputs(cols, cap, out):
    """The call's output arrays: `out` (a sequence of arrays of at least cap entries, e.g. from Engine.host_alloc) or
    fresh pageable ones; none at all for cap == 0."""
    if cap == 0 and out is None:
        return [None] * len(cols)
    if out is None:
        return [np.zeros(cap, dt) for _, dt in cols]
    out = list(out)
    if len(out) != len(cols) or any(a.dtype != dt or a.shape[0] < cap or not a.flags.c_contiguous
                                    for a, (_, dt) in zip(out, cols)):
        raise ValueError("out: one contiguous array of the column's dtype and at least cap entries per column")
    return out


def _nodes(nodes):
    a = np.ascontiguousarray(list(nodes), dtype=np.int32)
    return (_p(a) if a.size else None), int(a.size), a


def _finish(e, rc, name, outs, counts, cap):
    e.lib.check(rc, name)
    k = max(0, min(int(counts.n_hits), cap))
    return tuple(None if a is None else a[:k] for a in outs), counts


def election_scan_hits(e: Engine, gidx=None, down_nodes=(), long_dead_nodes=(), force=False, cap=None, n=None,
                       out=None):
    """gpx_election_scan_hits: ((gidx, run, bnum, first) of the groups that must run, ScanCounts).  gidx None = groups
    0 .. n-1 (n None: the whole table); cap None = n."""
    n, g = _scanned(e, gidx, n)
    cap = n if cap is None else int(cap)
    outs = _outputs(ELECTION_COLS, cap, out)
    dn, n_dn, _k1 = _nodes(down_nodes)
    ld, n_ld, _k2 = _nodes(long_dead_nodes)
    counts = ScanCounts()
    rc = e.lib.fn["election_scan_hits"](e.h, n, _p(g), dn, n_dn, ld, n_ld, int(bool(force)), cap,
                                        *[_p(a) for a in outs], C.byref(counts))
    return _finish(e, rc, "election_scan_hits", outs, counts, cap)


def poke_scan_hits(e: Engine, gidx=None, cap=None, n=None, out=None):
    """gpx_poke_scan_hits: ((gidx, poke, slot, bnum, bcoord, median_cp, flags, heard) of what waits for replies,
    ScanCounts)."""
    n, g = _scanned(e, gidx, n)
    cap = n if cap is None else int(cap)
    outs = _outputs(POKE_COLS, cap, out)
    counts = ScanCounts()
    rc = e.lib.fn["poke_scan_hits"](e.h, n, _p(g), cap, *[_p(a) for a in outs], C.byref(counts))
    return _finish(e, rc, "poke_scan_hits", outs, counts, cap)


def gap_scan_hits(e: Engine, gidx=None, threshold=1, sync_mode=SYNC_DEFAULT, size_limit=64, require=GAP_HIT_SYNC,
                  cap=None, n=None, out=None):
    """gpx_gap_scan_hits: ((gidx, first, max_committed, missing, sync) of the groups that satisfy every condition in
    `require` (GAP_HIT_*), ScanCounts)."""
    n, g = _scanned(e, gidx, n)
    cap = n if cap is None else int(cap)
    outs = _outputs(GAP_COLS, cap, out)
    counts = ScanCounts()
    rc = e.lib.fn["gap_scan_hits"](e.h, n, _p(g), int(threshold), int(sync_mode), int(size_limit), int(require), cap,
                                   *[_p(a) for a in outs], C.byref(counts))
    return _finish(e, rc, "gap_scan_hits", outs, counts, cap)


def _v(p):
    return _VP(int(p)) if p else None


def election_scan_hits_dev(e: Engine, n, gidx_ptr, down_nodes, long_dead_nodes, force, cap, out_ptrs, counts_ptr):
    """gpx_election_scan_hits_dev: gidx_ptr, the four out_ptrs (o_gidx, o_run, o_bnum, o_first) and counts_ptr are
    integer device addresses (0 = NULL); the node lists are host sequences.  Asynchronous."""
    dn, n_dn, _k1 = _nodes(down_nodes)
    ld, n_ld, _k2 = _nodes(long_dead_nodes)
    e.lib.check(e.lib.fn["election_scan_hits_dev"](e.h, int(n), _v(gidx_ptr), dn, n_dn, ld, n_ld, int(bool(force)),
                                                   int(cap), *[_v(p) for p in out_ptrs], _v(counts_ptr)),
                "election_scan_hits_dev")


def poke_scan_hits_dev(e: Engine, n, gidx_ptr, cap, out_ptrs, counts_ptr):
    """gpx_poke_scan_hits_dev: out_ptrs = o_gidx, o_poke, o_slot, o_bnum, o_bcoord, o_median_cp, o_flags, o_heard."""
    e.lib.check(e.lib.fn["poke_scan_hits_dev"](e.h, int(n), _v(gidx_ptr), int(cap), *[_v(p) for p in out_ptrs],
                                               _v(counts_ptr)), "poke_scan_hits_dev")


def gap_scan_hits_dev(e: Engine, n, gidx_ptr, threshold, sync_mode, size_limit, require, cap, out_ptrs, counts_ptr):
    """gpx_gap_scan_hits_dev: out_ptrs = o_gidx, o_first, o_max_committed, o_missing, o_sync."""
    e.lib.check(e.lib.fn["gap_scan_hits_dev"](e.h, int(n), _v(gidx_ptr), int(threshold), int(sync_mode),
                                              int(size_limit), int(require), int(cap), *[_v(p) for p in out_ptrs],
                                              _v(counts_ptr)), "gap_scan_hits_dev")


def election_begin_hits_dev(e: Engine, cap, counts_ptr, gidx_ptr, bnum_ptr, e_status_ptr):
    """gpx_election_begin_hits_dev: gpx_election_begin_dev for the first min(counts->n_hits, cap) entries, the count
    read on the device (integer device addresses)."""
    e.lib.check(e.lib.fn["election_begin_hits_dev"](e.h, int(cap), _v(counts_ptr), _v(gidx_ptr), _v(bnum_ptr),
                                                    _v(e_status_ptr)), "election_begin_hits_dev")
