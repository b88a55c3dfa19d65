"""The view change in list form (include/gpx_viewchange.h): the host side.

`prepare_lists` answers a batch of PREPAREs with the accepted pvalues as lists (pv_off, pv_slot, pv_bnum, pv_bcoord),
column for column the pvalue input of the coordinator calls; `prepare_reply_lists` applies a batch of PREPARE replies and
returns one row per HIT (ELECTED, PREEMPTED or a dropped record) plus one row per list entry; `prepare_reply_lists_more`
continues a cut call and `reply_lists_all` loops it to the end.  The `_dev` forms take integer device addresses
(0 = NULL) and queue the work on the engine's stream.  The signatures are registered in `_abi._DEV_SIGS` (HIP library
only: the CPU oracle has the dense calls, which are the specification of these)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._abi import Engine, PlCounts, PrlCounts, _i32, _p, _VP  # noqa: F401  (the counts: part of this module's interface)

VCL_TILE = 256  # GPX_VCL_TILE
HIT_COLS = (("rec", np.int32), ("gidx", np.int32), ("kind", np.uint8), ("status", np.uint8), ("median", np.int32),
            ("off", np.int32), ("count", np.int32))
ENTRY_COLS = (("slot", np.int32), ("kind", np.uint8), ("handle", np.int64), ("flags", np.uint8))
HIT_BYTES, ENTRY_BYTES, PV_BYTES = 22, 14, 12
COUNTS_BYTES = C.sizeof(PrlCounts)


@dataclass
class PrepareLists:
    """What gpx_prepare_lists returns: the dense reply columns, the lists cut to what was written, the counts."""
    r_bnum: np.ndarray
    r_bcoord: np.ndarray
    r_gc: np.ndarray
    r_flags: np.ndarray
    status: np.ndarray
    pv_off: np.ndarray  # recs_done + 1 entries
    pv_slot: np.ndarray
    pv_bnum: np.ndarray
    pv_bcoord: np.ndarray
    counts: PlCounts


@dataclass
class ReplyLists:
    """What gpx_prepare_reply_lists[_more] returns: hit and entry columns cut to what was written, the counts, and for
    the first call the dense v_kind / status columns (None where not asked for)."""
    hits: dict
    entries: dict
    counts: PrlCounts
    v_kind: np.ndarray | None = None
    status: np.ndarray | None = None


def _cols(cols, cap):
    return [np.zeros(cap, dt) if cap > 0 else None for _, dt in cols]


def prepare_lists(e: Engine, gidx, bnum, bcoord, first_slot, cap_entries=None) -> PrepareLists:
    """gpx_prepare_lists.  cap_entries None = n * window (never cuts); 0 counts only."""
    g = _i32(gidx)
    n = g.shape[0]
    bn, bc, fs = (_i32(x, n) for x in (bnum, bcoord, first_slot))
    cap = n * int(e.cfg.window) if cap_entries is None else int(cap_entries)
    m = max(n, 1)
    rb, rc, rg = (np.zeros(m, np.int32) for _ in range(3))
    rf, st = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    off = np.zeros(n + 1, np.int32)
    ps, pb, pc = (np.zeros(cap, np.int32) if cap > 0 else None for _ in range(3))
    counts = PlCounts()
    e.lib.check(e.lib.fn["prepare_lists"](e.h, n, _p(g), _p(bn), _p(bc), _p(fs), _p(rb), _p(rc), _p(rg), _p(rf), _p(st),
                                          cap, _p(off), _p(ps), _p(pb), _p(pc), C.byref(counts)), "prepare_lists")
    k = max(0, min(int(counts.entries_done), cap))
    empty = np.zeros(0, np.int32)
    return PrepareLists(rb[:n], rc[:n], rg[:n], rf[:n], st[:n], off[:int(counts.recs_done) + 1],
                        *(empty if a is None else a[:k] for a in (ps, pb, pc)), counts)


def _pvalue_columns(n, pvalues):
    """(pv_off, slot, bnum, bcoord, handle, flags) from per-record lists of (slot, bnum, bcoord, handle, flags) tuples,
    or from a tuple of ready columns."""
    if isinstance(pvalues, tuple) and len(pvalues) == 6:
        off, ps, pb, pc, ph, pf = pvalues
        return (_i32(off, n + 1), _i32(ps), _i32(pb), _i32(pc),
                None if ph is None else np.ascontiguousarray(ph, np.int64),
                None if pf is None else np.ascontiguousarray(pf, np.uint8))
    pvalues = pvalues if pvalues is not None else [[] for _ in range(n)]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pvalues])
    flat = [t for p in pvalues for t in p]
    m = max(len(flat), 1)
    ps, pb, pc = (np.zeros(m, np.int32) for _ in range(3))
    ph, pf = np.zeros(m, np.int64), np.zeros(m, np.uint8)
    for j, t in enumerate(flat):
        ps[j], pb[j], pc[j], ph[j], pf[j] = t
    return off, ps, pb, pc, ph, pf


def _cut(hcols, ecols, counts, cap_hits, cap_entries):
    kh = max(0, min(int(counts.hits_done), cap_hits))
    ke = max(0, min(int(counts.entries_done), cap_entries))
    hits = {name: (np.zeros(0, dt) if a is None else a[:kh]) for (name, dt), a in zip(HIT_COLS, hcols)}
    entries = {name: (np.zeros(0, dt) if a is None else a[:ke]) for (name, dt), a in zip(ENTRY_COLS, ecols)}
    return hits, entries


def prepare_reply_lists(e: Engine, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues=None, cap_hits=None,
                        cap_entries=None, dense=True) -> ReplyLists:
    """gpx_prepare_reply_lists.  cap_hits None = n, cap_entries None = n * window (never cut); dense: also fetch the
    v_kind / status columns."""
    g = _i32(gidx)
    n = g.shape[0]
    ac, rb, rc, fs = (_i32(x, n) for x in (acceptor, r_bnum, r_bcoord, first_slot))
    off, ps, pb, pc, ph, pf = _pvalue_columns(n, pvalues)
    ch = n if cap_hits is None else int(cap_hits)
    ce = n * int(e.cfg.window) if cap_entries is None else int(cap_entries)
    vk = np.zeros(max(n, 1), np.uint8) if dense else None
    st = np.zeros(max(n, 1), np.uint8) if dense else None
    hcols, ecols = _cols(HIT_COLS, ch), _cols(ENTRY_COLS, ce)
    counts = PrlCounts()
    e.lib.check(e.lib.fn["prepare_reply_lists"](e.h, n, _p(g), _p(ac), _p(rb), _p(rc), _p(fs), _p(off), _p(ps), _p(pb),
                                                _p(pc), _p(ph), _p(pf), _p(vk), _p(st), ch, ce,
                                                *[_p(a) for a in hcols], *[_p(a) for a in ecols], C.byref(counts)),
                "prepare_reply_lists")
    hits, entries = _cut(hcols, ecols, counts, ch, ce)
    return ReplyLists(hits, entries, counts, None if vk is None else vk[:n], None if st is None else st[:n])


def prepare_reply_lists_more(e: Engine, from_hit, cap_hits, cap_entries) -> ReplyLists:
    """gpx_prepare_reply_lists_more: the hits from `from_hit` on of the last prepare_reply_lists call."""
    ch, ce = int(cap_hits), int(cap_entries)
    hcols, ecols = _cols(HIT_COLS, ch), _cols(ENTRY_COLS, ce)
    counts = PrlCounts()
    e.lib.check(e.lib.fn["prepare_reply_lists_more"](e.h, int(from_hit), ch, ce, *[_p(a) for a in hcols],
                                                     *[_p(a) for a in ecols], C.byref(counts)),
                "prepare_reply_lists_more")
    hits, entries = _cut(hcols, ecols, counts, ch, ce)
    return ReplyLists(hits, entries, counts)


def reply_lists_all(e: Engine, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues=None, cap_hits=None,
                    cap_entries=None, dense=True) -> ReplyLists:
    """prepare_reply_lists, then prepare_reply_lists_more until every hit has been returned: the complete lists, h_off
    relative to the concatenated entry columns.  cap_entries must be at least the window (the progress guarantee)."""
    first = prepare_reply_lists(e, gidx, acceptor, r_bnum, r_bcoord, first_slot, pvalues, cap_hits, cap_entries, dense)
    n = len(first.v_kind) if first.v_kind is not None else len(_i32(gidx))
    ch = n if cap_hits is None else int(cap_hits)
    ce = n * int(e.cfg.window) if cap_entries is None else int(cap_entries)
    parts, done, ents = [first], int(first.counts.hits_done), int(first.counts.entries_done)
    while done < int(first.counts.n_hits):
        r = prepare_reply_lists_more(e, done, ch, ce)
        if int(r.counts.hits_done) == 0:
            raise ValueError("reply_lists_all: the caps admit no further hit (cap_hits >= 1 and cap_entries >= window)")
        r.hits["off"] = r.hits["off"] + np.int32(ents)
        parts.append(r)
        done += int(r.counts.hits_done)
        ents += int(r.counts.entries_done)
    hits = {name: np.concatenate([p.hits[name] for p in parts]) for name, _ in HIT_COLS}
    entries = {name: np.concatenate([p.entries[name] for p in parts]) for name, _ in ENTRY_COLS}
    counts = PrlCounts.from_buffer_copy(bytes(first.counts))
    counts.hits_done, counts.entries_done = done, ents
    return ReplyLists(hits, entries, counts, first.v_kind, first.status)


def _v(p):
    return _VP(int(p)) if p else None


def prepare_lists_dev(e: Engine, n, in_ptrs, dense_ptrs, cap_entries, list_ptrs, counts_ptr):
    """gpx_prepare_lists_dev: in_ptrs = gidx, bnum, bcoord, first_slot; dense_ptrs = r_bnum, r_bcoord, r_gc, r_flags,
    status; list_ptrs = pv_off, pv_slot, pv_bnum, pv_bcoord (integer device addresses).  Asynchronous."""
    e.lib.check(e.lib.fn["prepare_lists_dev"](e.h, int(n), *[_v(p) for p in in_ptrs], *[_v(p) for p in dense_ptrs],
                                              int(cap_entries), *[_v(p) for p in list_ptrs], _v(counts_ptr)),
                "prepare_lists_dev")


def prepare_reply_lists_dev(e: Engine, n, in_ptrs, pv_total, pv_ptrs, v_kind_ptr, status_ptr, cap_hits, cap_entries,
                            hit_ptrs, entry_ptrs, counts_ptr):
    """gpx_prepare_reply_lists_dev: in_ptrs = gidx, acceptor, r_bnum, r_bcoord, first_slot, pv_off; pv_ptrs = pv_slot,
    pv_bnum, pv_bcoord, pv_handle, pv_flags; hit_ptrs = the seven h_* columns; entry_ptrs = the four e_* columns."""
    e.lib.check(e.lib.fn["prepare_reply_lists_dev"](e.h, int(n), *[_v(p) for p in in_ptrs], int(pv_total),
                                                    *[_v(p) for p in pv_ptrs], _v(v_kind_ptr), _v(status_ptr),
                                                    int(cap_hits), int(cap_entries), *[_v(p) for p in hit_ptrs],
                                                    *[_v(p) for p in entry_ptrs], _v(counts_ptr)),
                "prepare_reply_lists_dev")


def prepare_reply_lists_more_dev(e: Engine, from_hit, cap_hits, cap_entries, hit_ptrs, entry_ptrs, counts_ptr):
    """gpx_prepare_reply_lists_more_dev."""
    e.lib.check(e.lib.fn["prepare_reply_lists_more_dev"](e.h, int(from_hit), int(cap_hits), int(cap_entries),
                                                         *[_v(p) for p in hit_ptrs], *[_v(p) for p in entry_ptrs],
                                                         _v(counts_ptr)), "prepare_reply_lists_more_dev")
