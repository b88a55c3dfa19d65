"""Group images (include/gpx_image.h): the host side.

`export_groups` / `import_groups` are the host-pointer calls; `export_groups_dev` / `import_groups_dev` take integer
device addresses (0 = NULL) and queue the call on the engine's stream.  `rows_to_dumps` turns rows into the canonical
words of gpx_group_dump, `move_groups` takes live groups from one engine to another through device memory.  The
signatures are registered in `_abi._DEV_SIGS` / `_HOST_SIGS` (HIP library only: the CPU oracle's group_dump,
group_snapshot and group_create are the specification of these).

Delta images (include/gpx_delta.h): `export_delta` / `apply_delta` and their `_dev` forms move only the groups that
changed since the export that last wrote them; `mirror_groups` keeps a second engine current through device memory."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import Engine, GpxError, S_OK, S_NOGROUP, load_hip, _i32, _p, _VP

IMAGE_FORMAT, IMAGE_MAIN, IMAGE_CONT, HEADER_WORDS = 1, 1, 2, 16
IMAGE_TILE = 256                          # GPX_IMAGE_TILE_ENTRIES: entries or rows per workgroup
F_EXISTS, F_STOPPED, F_HASCOORD, F_PREPARING, F_CONTINUED, F_K_SHIFT = 1, 2, 4, 8, 16, 8
P_PRESENT, P_STOP = 0x10000, 0x20000
R_PRESENT, R_STOP, R_HASVALUE = 1, 2, 4
CO_PRESENT = 0x100
IMG_EVICT, IMG_VIEWCHANGE = 1, 2
S_IMAGE = 10
COUNTS_BYTES = 16

# the 16 header words of a row (a continuation row uses format, kind, gidx and - in the place of version - c_wait)
IMAGE_HEADER_DTYPE = np.dtype([
    ("format", "<i4"), ("kind", "<i4"), ("flags", "<u4"), ("my_id", "<i4"), ("kmax", "<u2"), ("window", "<u2"),
    ("gidx", "<i4"), ("version", "<i4"), ("a_slot", "<i4"), ("a_bnum", "<i4"), ("a_bcoord", "<i4"), ("a_gc", "<i4"),
    ("c_bnum", "<i4"), ("c_bcoord", "<i4"), ("c_next", "<i4"), ("c_pcount", "<i4"), ("reserved", "<i4")])
assert IMAGE_HEADER_DTYPE.itemsize == 4 * HEADER_WORDS


class ImageCounts(C.Structure):
    """struct gpx_image_counts (include/gpx_image.h)."""
    _fields_ = [("n_live", C.c_int32), ("n_rows", C.c_int32), ("n_done", C.c_int32), ("n_rows_done", C.c_int32)]

    def as_tuple(self):
        return (self.n_live, self.n_rows, self.n_done, self.n_rows_done)


def image_stride(kmax: int, window: int, lib=None) -> int:
    """gpx_image_stride: bytes per row, -1 for a shape no engine can have."""
    return int((lib or load_hip()).fn["image_stride"](int(kmax), int(window)))


def _stride(e: Engine) -> int:
    return image_stride(int(e.cfg.kmax), int(e.cfg.window), e.lib)


def export_groups(e: Engine, gidx=None, flags=0, cap=None, n=None, out=None):
    """gpx_group_export: (rows written as a uint8 array [n_rows_done, stride], ImageCounts).  gidx None = groups
    0 .. n-1 (n None: the whole table).  cap None = whatever the entries need (one counting call first); `out`: a
    contiguous uint8 array of at least cap * stride bytes to write into instead of a fresh one; cap == 0 without `out`
    passes a null buffer and only counts."""
    if gidx is None:
        n, g = (int(e.cfg.max_groups) if n is None else int(n)), None
    else:
        g = _i32(gidx)
        n = g.shape[0]
    stride = _stride(e)
    counts = ImageCounts()
    fn = e.lib.fn["group_export"]
    if cap is None:
        e.lib.check(fn(e.h, n, _p(g), 0, 0, None, C.byref(counts)), "group_export")
        cap = int(counts.n_rows)
    cap = int(cap)
    if out is None:
        out = np.zeros(cap * stride, np.uint8) if cap else None
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < cap * stride:
        raise ValueError("out: a contiguous uint8 array of at least cap * stride bytes")
    e.lib.check(fn(e.h, n, _p(g), int(flags), cap, _p(out), C.byref(counts)), "group_export")
    k = int(counts.n_rows_done)
    rows = np.zeros((0, stride), np.uint8) if out is None else out.reshape(-1)[:k * stride].reshape(k, stride)
    return rows, counts


def import_groups(e: Engine, rows, gidx=None, flags=0):
    """gpx_group_import: the status of every row.  rows: uint8 [n_rows, stride] (or flat); gidx None = every group goes
    to its source gidx."""
    stride = _stride(e)
    rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1, stride)
    n = rows.shape[0]
    g = None if gidx is None else _i32(gidx, n)
    status = np.zeros(max(n, 1), np.uint8)
    e.lib.check(e.lib.fn["group_import"](e.h, n, _p(rows), _p(g), int(flags), _p(status)), "group_import")
    return status[:n]


def _v(p):
    return _VP(int(p)) if p else None


def export_groups_dev(e: Engine, n, gidx_ptr, flags, cap, rows_ptr, counts_ptr):
    """gpx_group_export_dev: gidx_ptr, rows_ptr and counts_ptr are integer device addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["group_export_dev"](e.h, int(n), _v(gidx_ptr), int(flags), int(cap), _v(rows_ptr), _v(counts_ptr)),
                "group_export_dev")


def import_groups_dev(e: Engine, n_rows, rows_ptr, gidx_ptr, flags, status_ptr):
    """gpx_group_import_dev: rows_ptr, gidx_ptr and status_ptr are integer device addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["group_import_dev"](e.h, int(n_rows), _v(rows_ptr), _v(gidx_ptr), int(flags), _v(status_ptr)),
                "group_import_dev")


def layout(kmax: int, window: int) -> dict:
    """word offsets of the sections of a main and of a continuation row, and the stride in words"""
    K, W = int(kmax), int(window)
    o_mem = HEADER_WORDS
    o_ns, o_p = o_mem + K, o_mem + 2 * K
    o_acc = o_p + W
    o_com = o_acc + 4 * W
    return dict(mem=o_mem, ns=o_ns, p=o_p, acc=o_acc, com=o_com, co=HEADER_WORDS, coh=HEADER_WORDS + 4 * W,
                ph=HEADER_WORDS + 6 * W, stride_w=(o_com + 4 * W + 15) // 16 * 16)


def rows_to_dumps(rows, kmax: int, window: int):
    """The canonical dump words of gpx_group_dump (docs/HISTORY.md, state dump) of every group in `rows`: one int32
    array per main row, in row order; a continuation row goes into the dump of the main row before it."""
    K, W = int(kmax), int(window)
    L = layout(K, W)
    w = np.ascontiguousarray(rows).view(np.uint8).reshape(-1, 4 * L["stride_w"]).view("<i4").astype(np.int64)
    dumps, j = [], 0
    while j < w.shape[0]:
        r = w[j]
        if r[0] != IMAGE_FORMAT or r[1] != IMAGE_MAIN:
            raise ValueError(f"row {j}: not a main row")
        fl = int(r[2])
        k = (fl >> F_K_SHIFT) & 0xff
        d = [1, int(r[6]), k] + r[L["mem"]:L["mem"] + k].tolist() + r[7:11].tolist() + [1 if fl & F_STOPPED else 0]
        acc = r[L["acc"]:L["acc"] + 4 * W].reshape(W, 4)
        com = r[L["com"]:L["com"] + 4 * W].reshape(W, 4)
        ent = sorted((int(a[0]), int(a[1]), int(a[2]), 1 if a[3] & R_STOP else 0) for a in acc if a[3] & R_PRESENT)
        d += [len(ent)] + [x for t in ent for x in t]
        ent = sorted((int(c[0]), int(c[1]), int(c[2]), int(c[3]), 1 if (a[3] >> 8) & R_HASVALUE else 0,
                      1 if (a[3] >> 8) & R_STOP else 0) for a, c in zip(acc, com) if (a[3] >> 8) & R_PRESENT)
        d += [len(ent)] + [x for t in ent for x in t]
        d.append(1 if fl & F_HASCOORD else 0)
        cont = None
        if fl & F_CONTINUED:
            j += 1
            if j >= w.shape[0] or w[j][1] != IMAGE_CONT or w[j][5] != r[5]:
                raise ValueError(f"row {j}: the continuation row of row {j - 1} is missing")
            cont = w[j]
        if fl & F_HASCOORD:
            nxt = int(r[13])
            d += [int(r[11]), int(r[12]), nxt] + r[L["ns"]:L["ns"] + k].tolist()
            props = []
            for back in range(W, 0, -1):                      # slots next - W .. next - 1, in that order
                s = ((nxt - back + 2**31) % 2**32) - 2**31
                e = int(r[L["p"] + (s & (W - 1))])
                if e & P_PRESENT:
                    props.append((s, e))
            props.sort()
            d += [len(props)] + [x for s, e in props for x in (s, 1 if e & P_STOP else 0, e & 0xffff)]
            d.append(0 if fl & F_PREPARING else 1)
            if fl & F_PREPARING:
                d += [1, int(cont[6])]
                for s, _ in props:
                    d += cont[L["ph"] + 2 * (s & (W - 1)):L["ph"] + 2 * (s & (W - 1)) + 2].tolist()
                co = cont[L["co"]:L["co"] + 4 * W].reshape(W, 4)
                coh = cont[L["coh"]:L["coh"] + 2 * W].reshape(W, 2)
                ent = sorted((int(c[0]), int(c[1]), int(c[2]), int(c[3]) & 3, int(h[0]), int(h[1]))
                             for c, h in zip(co, coh) if c[3] & CO_PRESENT)
                d += [len(ent)] + [x for t in ent for x in t]
        dumps.append(np.array(d, np.int64).astype(np.int32))
        j += 1
    return dumps


def move_groups(src: Engine, dst: Engine, src_gidx, dst_gidx):
    """Takes the live groups src_gidx[i] of `src` to row dst_gidx[i] of `dst`: export with GPX_IMG_EVICT on `src`, import
    on `dst`, through device buffers - no row crosses the link (the counts and one status byte per entry do).  Both
    engines live on the current device and have the same kmax, window and my_id.  Entries and destinations must be
    pairwise distinct.  Returns one status per entry: GPX_S_NOGROUP for an entry that named no live group of `src`,
    otherwise what the import said.  A group whose import was refused is imported again into its source row of `src`:
    no group is ever lost."""
    import torch

    sg, dg = _i32(src_gidx), _i32(dst_gidx, len(src_gidx))
    n = sg.shape[0]
    out = np.full(n, S_NOGROUP, np.uint8)
    if n == 0:
        return out
    stride = _stride(src)
    if _stride(dst) != stride:
        raise ValueError("move_groups: the engines differ in kmax or window")
    dev = "cuda"
    rows = torch.empty((2 * n, stride // 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    t_sg, t_dg = torch.from_numpy(sg).to(dev), torch.from_numpy(dg).to(dev)
    torch.cuda.synchronize()
    export_groups_dev(src, n, t_sg.data_ptr(), IMG_EVICT, 2 * n, rows.data_ptr(), cnt.data_ptr())
    src.sync()
    n_live, n_rows, n_done, n_rows_done = cnt.cpu().tolist()
    assert n_done == n_live and n_rows_done == n_rows
    if n_rows == 0:
        return out
    rows = rows[:n_rows]
    # the destination of every row, from its source gidx word, on the device
    order = torch.argsort(t_sg)
    entry = order[torch.searchsorted(t_sg[order], rows[:, 5].contiguous())]
    t_rg = t_dg[entry].contiguous()
    status = torch.zeros(n_rows, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    flags = IMG_VIEWCHANGE if n_rows > n_live else 0
    import_groups_dev(dst, n_rows, rows.data_ptr(), t_rg.data_ptr(), flags, status.data_ptr())
    dst.sync()
    refused = status != S_OK
    if bool(refused.any()):
        back = rows[refused].contiguous()
        st2 = torch.zeros(back.shape[0], dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        import_groups_dev(src, back.shape[0], back.data_ptr(), 0, flags, st2.data_ptr())
        src.sync()
        if bool((st2 != S_OK).any()):
            raise GpxError("move_groups: a refused group could not be put back into its source row")
    main = rows[:, 1] == IMAGE_MAIN
    res = torch.full((n,), S_NOGROUP, dtype=torch.uint8, device=dev)
    res[entry[main]] = status[main]
    return res.cpu().numpy()


# ---- delta images (include/gpx_delta.h) ----
DELTA_EVICT, DELTA_FULL = 1, 2
DELTA_COUNTS_BYTES = 32


class DeltaCounts(C.Structure):
    """struct gpx_delta_counts (include/gpx_delta.h)."""
    _fields_ = [(f, C.c_int32) for f in ("n_live", "n_changed", "n_rows", "n_done", "n_rows_done", "n_gone", "n_gone_done",
                                         "reserved")]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


def export_delta(e: Engine, gidx=None, flags=0, cap=None, cap_gone=None, n=None, out=None, out_gone=None):
    """gpx_group_export_delta: (rows written as uint8 [n_rows_done, stride], the gone groups as int32 [n_gone_done],
    DeltaCounts).  gidx None = groups 0 .. n-1 (n None: the whole table).  cap / cap_gone None = whatever the entries
    need (one counting call first, which changes no mark); `out` / `out_gone`: contiguous arrays (uint8 of at least
    cap * stride bytes, int32 of at least cap_gone entries) to write into instead of fresh ones; a cap of 0 without its
    array passes a null buffer."""
    if gidx is None:
        n, g = (int(e.cfg.max_groups) if n is None else int(n)), None
    else:
        g = _i32(gidx)
        n = g.shape[0]
    stride = _stride(e)
    counts = DeltaCounts()
    fn = e.lib.fn["group_export_delta"]
    if cap is None or cap_gone is None:
        e.lib.check(fn(e.h, n, _p(g), int(flags) & DELTA_FULL, 0, None, 0, None, C.byref(counts)), "group_export_delta")
        cap = int(counts.n_rows) if cap is None else cap
        cap_gone = int(counts.n_gone) if cap_gone is None else cap_gone
    cap, cap_gone = int(cap), int(cap_gone)
    if out is None:
        out = np.zeros(cap * stride, np.uint8) if cap else None
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < cap * stride:
        raise ValueError("out: a contiguous uint8 array of at least cap * stride bytes")
    if out_gone is None:
        out_gone = np.zeros(cap_gone, np.int32) if cap_gone else None
    elif out_gone.dtype != np.int32 or not out_gone.flags.c_contiguous or out_gone.size < cap_gone:
        raise ValueError("out_gone: a contiguous int32 array of at least cap_gone entries")
    e.lib.check(fn(e.h, n, _p(g), int(flags), cap, _p(out), cap_gone, _p(out_gone), C.byref(counts)), "group_export_delta")
    k = int(counts.n_rows_done)
    rows = np.zeros((0, stride), np.uint8) if out is None else out.reshape(-1)[:k * stride].reshape(k, stride)
    gone = np.zeros(0, np.int32) if out_gone is None else out_gone.reshape(-1)[:int(counts.n_gone_done)]
    return rows, gone, counts


def apply_delta(e: Engine, rows, gidx=None, flags=0, gone=None):
    """gpx_group_apply_delta: (the status of every row, the status of every gone entry).  rows: uint8 [n_rows, stride]
    (or flat, or None); gidx None = every group goes to its source gidx."""
    stride = _stride(e)
    rows = np.zeros((0, stride), np.uint8) if rows is None else np.ascontiguousarray(rows).view(np.uint8).reshape(-1, stride)
    n = rows.shape[0]
    g = None if gidx is None else _i32(gidx, n)
    x = _i32([] if gone is None else gone)
    status, gstatus = np.zeros(max(n, 1), np.uint8), np.zeros(max(x.shape[0], 1), np.uint8)
    e.lib.check(e.lib.fn["group_apply_delta"](e.h, n, _p(rows) if n else None, _p(g), int(flags), _p(status), x.shape[0],
                                              _p(x) if x.shape[0] else None, _p(gstatus)), "group_apply_delta")
    return status[:n], gstatus[:x.shape[0]]


def export_delta_dev(e: Engine, n, gidx_ptr, flags, cap, rows_ptr, cap_gone, gone_ptr, counts_ptr):
    """gpx_group_export_delta_dev: the pointers are integer device addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["group_export_delta_dev"](e.h, int(n), _v(gidx_ptr), int(flags), int(cap), _v(rows_ptr), int(cap_gone),
                                                   _v(gone_ptr), _v(counts_ptr)), "group_export_delta_dev")


def apply_delta_dev(e: Engine, n_rows, rows_ptr, gidx_ptr, flags, status_ptr, n_gone, gone_ptr, gone_status_ptr):
    """gpx_group_apply_delta_dev: the pointers are integer device addresses (0 = NULL).  Asynchronous."""
    e.lib.check(e.lib.fn["group_apply_delta_dev"](e.h, int(n_rows), _v(rows_ptr), _v(gidx_ptr), int(flags), _v(status_ptr),
                                                  int(n_gone), _v(gone_ptr), _v(gone_status_ptr)), "group_apply_delta_dev")


def mirror_groups(src: Engine, dst: Engine, full=False):
    """Brings `dst` up to date with `src` over the whole table: one delta export on `src` (a baseline under `full`), one
    apply on `dst` at the same rows, through device buffers - only the counts and the status bytes cross the link.
    Both engines live on the current device and have the same max_groups, kmax, window and my_id.  The host must not
    feed `dst` groups that `src` owns.  Returns (DeltaCounts of the export, row statuses, gone statuses)."""
    import torch

    stride = _stride(src)
    if _stride(dst) != stride or int(dst.cfg.max_groups) != int(src.cfg.max_groups):
        raise ValueError("mirror_groups: the engines differ in max_groups, kmax or window")
    n = int(src.cfg.max_groups)
    dev = "cuda"
    cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fl = DELTA_FULL if full else 0
    export_delta_dev(src, n, 0, fl, 0, 0, 0, 0, cnt.data_ptr())          # count: changes no mark
    src.sync()
    c = cnt.cpu().tolist()
    n_rows, n_gone = c[2], c[5]
    rows = torch.empty((max(n_rows, 1), stride // 4), dtype=torch.int32, device=dev)
    gone = torch.empty(max(n_gone, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    export_delta_dev(src, n, 0, fl, n_rows, rows.data_ptr() if n_rows else 0, n_gone, gone.data_ptr() if n_gone else 0,
                     cnt.data_ptr())
    src.sync()
    counts = DeltaCounts(*cnt.cpu().tolist())
    assert counts.n_rows_done == n_rows and counts.n_gone_done == n_gone
    status = torch.zeros(max(n_rows, 1), dtype=torch.uint8, device=dev)
    gstatus = torch.zeros(max(n_gone, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    apply_delta_dev(dst, n_rows, rows.data_ptr() if n_rows else 0, 0, IMG_VIEWCHANGE if n_rows > counts.n_done else 0,
                    status.data_ptr(), n_gone, gone.data_ptr() if n_gone else 0, gstatus.data_ptr())
    dst.sync()
    return counts, status[:n_rows].cpu().numpy(), gstatus[:n_gone].cpu().numpy()
