"""numpy restatement of include/gpx_packed_out.h: the packing rule (reference entry, rows, form), the layout of both
forms and their reading, written from the header's text and independent of the library's code.  Also the columns and
the engine inputs the packed-output tests share."""
import numpy as np

from gigapaxos_amd import hri_create, streams

RECORDS, COLUMNS = 1, 2
DECISIONS, PROPOSALS = 1, 2
EXC_BIT = 0x80000000
RESERVED = {DECISIONS: 0x7FFC0000, PROPOSALS: 0x7F000000}
M32 = 0xFFFFFFFF
REF_WINDOW = 64


def R(x):
    return (int(x) + 31) // 32 * 32


def out_bytes(cap):
    """GPX_PACKED_OUT_BYTES"""
    return 32 + 5 * R(4 * cap) + R(cap)


def _i32(x):
    return (np.asarray(x, np.int64) & M32).astype(np.uint32).view(np.int32)


def _split(kind, cols):
    """-> (gidx or None, slot, bnum, bcoord, cp, byte column) from the columns in the order of include/gpx.h"""
    if kind == DECISIONS:
        g, sl, bn, bc, cp, b = cols
    else:
        g = None
        sl, bn, bc, cp, b = cols
    i = lambda c: np.asarray(c, np.int32)  # noqa: E731
    return (None if g is None else i(g)), i(sl), i(bn), i(bc), i(cp), np.asarray(b, np.uint8)


def reference(bnum, bcoord):
    """Index of the reference entry, or None for an empty call: among the first min(n, 64) entries the ballot that
    occurs most often, on a tie the one first seen earliest; the reference is that ballot's first occurrence."""
    seen = {}
    for i, b in enumerate(zip(bnum[:REF_WINDOW].tolist(), bcoord[:REF_WINDOW].tolist())):
        first, cnt = seen.get(b, (i, 0))
        seen[b] = (first, cnt + 1)
    if not seen:
        return None
    return min(seen.values(), key=lambda fc: (-fc[1], fc[0]))[0]


def rule(kind, cols):
    """-> (header dict, needs-a-row mask, dslot, dcp)"""
    _, sl, bn, bc, cp, _ = _split(kind, cols)
    n = sl.shape[0]
    ref = reference(bn, bc)
    if ref is None:
        return dict(form=RECORDS, kind=kind, n=0, n_exc=0, bnum=0, bcoord=0, base_slot=0, base_cp=0), np.zeros(0, bool), None, None
    base_slot, base_cp = (int(sl[ref]) - 128) & M32, (int(cp[ref]) - 128) & M32
    ds = (sl.astype(np.int64) - base_slot) & M32
    dp = (cp.astype(np.int64) - base_cp) & M32
    need = (bn != bn[ref]) | (bc != bc[ref]) | (ds > 255) | (dp > 255)
    needed = int(need.sum())
    rec = needed <= n // 4
    hdr = dict(form=RECORDS if rec else COLUMNS, kind=kind, n=n, n_exc=needed if rec else 0, bnum=int(bn[ref]),
               bcoord=int(bc[ref]), base_slot=int(_i32(base_slot)), base_cp=int(_i32(base_cp)))
    return hdr, need, ds, dp


def needed_rows(kind, cols):
    return int(rule(kind, cols)[1].sum())


def used_size(hdr):
    n, S = hdr["n"], R(4 * hdr["n"])
    if hdr["form"] == RECORDS:
        return 32 + (R(8 * n) if hdr["kind"] == DECISIONS else S) + 32 * hdr["n_exc"]
    return 32 + (5 if hdr["kind"] == DECISIONS else 4) * S + R(n)


def pack(kind, cols):
    """-> (uint8 array of exactly the used size, header dict, rows needed)"""
    g, sl, bn, bc, cp, b = _split(kind, cols)
    hdr, need, ds, dp = rule(kind, cols)
    n = hdr["n"]
    out = np.zeros(used_size(hdr), np.uint8)
    out[:32].view(np.int32)[:] = [hdr[f] for f in ("form", "kind", "n", "n_exc", "bnum", "bcoord", "base_slot", "base_cp")]
    if n == 0:
        return out, hdr, 0
    S = R(4 * n)
    if hdr["form"] == RECORDS:
        w = (ds & 255) | ((dp & 255) << 8) | (b.astype(np.int64) << 16)
        ex = np.nonzero(need)[0]
        w[ex] = EXC_BIT | np.arange(ex.shape[0])
        w = w.astype(np.uint32)
        if kind == DECISIONS:
            rec = out[32:32 + 8 * n].view(np.uint32).reshape(n, 2)
            rec[:, 0] = g.view(np.uint32)
            rec[:, 1] = w
            at = 32 + R(8 * n)
            fields = (bn, bc, sl, cp, b)
        else:
            out[32:32 + 4 * n].view(np.uint32)[:] = w
            at = 32 + S
            fields = (sl, bn, bc, cp, b)
        rows = out[at:at + 32 * ex.shape[0]].view(np.int32).reshape(-1, 8)
        for k, c in enumerate(fields):
            rows[:, k] = c[ex]
    else:
        icols = (g, sl, bn, bc, cp) if kind == DECISIONS else (sl, bn, bc, cp)
        for k, c in enumerate(icols):
            out[32 + k * S:32 + k * S + 4 * n].view(np.int32)[:] = c
        at = 32 + len(icols) * S
        out[at:at + n] = b
    return out, hdr, int(need.sum())


def unpack(kind, buf):
    """-> the plain columns in the order of include/gpx.h; raises ValueError for a buffer that is not self-consistent"""
    buf = np.asarray(buf, np.uint8)
    if buf.shape[0] < 32:
        raise ValueError("no header")
    h = buf[:32].view(np.int32)
    hdr = dict(zip(("form", "kind", "n", "n_exc", "bnum", "bcoord", "base_slot", "base_cp"), (int(x) for x in h)))
    n, n_exc = hdr["n"], hdr["n_exc"]
    if hdr["kind"] != kind or hdr["form"] not in (RECORDS, COLUMNS) or n < 0 or n_exc < 0:
        raise ValueError("header")
    if hdr["form"] == COLUMNS and n_exc:
        raise ValueError("rows in the columns form")
    if used_size(hdr) > buf.shape[0]:
        raise ValueError("size beyond the buffer")
    S = R(4 * n)
    nc = 5 if kind == DECISIONS else 4
    if hdr["form"] == COLUMNS:
        cols = [buf[32 + k * S:32 + k * S + 4 * n].view(np.int32).copy() for k in range(nc)]
        return tuple(cols) + (buf[32 + nc * S:32 + nc * S + n].copy(),)
    if kind == DECISIONS:
        rec = buf[32:32 + 8 * n].view(np.uint32).reshape(n, 2)
        g, w = rec[:, 0].view(np.int32).copy(), rec[:, 1]
        at = 32 + R(8 * n)
    else:
        g, w = None, buf[32:32 + 4 * n].view(np.uint32)
        at = 32 + S
    rows = buf[at:at + 32 * n_exc].view(np.int32).reshape(-1, 8)
    is_exc = (w & EXC_BIT) != 0
    r = (w & ~np.uint32(EXC_BIT)).astype(np.int64)
    if (is_exc & (r >= n_exc)).any() or (~is_exc & ((w & RESERVED[kind]) != 0)).any():
        raise ValueError("record")
    w64 = w.astype(np.int64)
    row = rows[np.where(is_exc, r, 0)] if n_exc else np.zeros((n, 8), np.int32)
    d_sl = _i32((hdr["base_slot"] & M32) + (w64 & 255))
    d_cp = _i32((hdr["base_cp"] & M32) + ((w64 >> 8) & 255))
    d_b = ((w64 >> 16) & 255).astype(np.uint8)
    ks, kn, kc = (2, 0, 1) if kind == DECISIONS else (0, 1, 2)
    sl = np.where(is_exc, row[:, ks], d_sl).astype(np.int32)
    bn = np.where(is_exc, row[:, kn], hdr["bnum"]).astype(np.int32)
    bc = np.where(is_exc, row[:, kc], hdr["bcoord"]).astype(np.int32)
    cp = np.where(is_exc, row[:, 3], d_cp).astype(np.int32)
    b = np.where(is_exc, row[:, 4].astype(np.uint8), d_b).astype(np.uint8)
    return ((g,) if kind == DECISIONS else ()) + (sl, bn, bc, cp, b)


# ---- synthetic columns ------------------------------------------------------------------------------------------
def steady(kind, n, slot=7, cp=6, byte=None):
    """n entries of one ballot (0, 100) at one slot: what a steady round gives"""
    b = np.full(n, 1 if kind == DECISIONS else 0, np.uint8) if byte is None else np.asarray(byte, np.uint8)
    cols = [np.full(n, slot, np.int32), np.zeros(n, np.int32), np.full(n, 100, np.int32), np.full(n, cp, np.int32), b]
    return ([np.arange(n, dtype=np.int32)] if kind == DECISIONS else []) + cols


def with_rows(kind, n, rows_at):
    """steady columns with the entries `rows_at` at a far slot: exactly len(rows_at) rows"""
    cols = steady(kind, n)
    cols[1 if kind == DECISIONS else 0][np.asarray(rows_at, np.int64)] = 100_000
    return cols


def synthetic_cases(kind):
    rng = np.random.default_rng(77 + kind)
    o = 1 if kind == DECISIONS else 0  # index of the slot column
    out = {}
    for name, around in (("straddles MAX_VALUE", 2**31 - 1), ("straddles MIN_VALUE", -2**31)):
        c = steady(kind, 5000)
        c[o] = _i32(around + rng.integers(-50, 50, 5000))
        c[o + 3] = _i32(around - 1 + rng.integers(-50, 50, 5000))
        out[name] = c
    c = steady(kind, 2000)                                   # an odd first entry: another ballot, a far slot
    c[o][0], c[o + 1][0], c[o + 2][0] = 1 << 30, 9, 101
    out["odd first entry"] = c
    c = steady(kind, 500)                                    # 32 : 32 among the first 64; the later majority must not matter
    c[o + 2][0:64:2] = 101
    c[o + 2][64:] = 100
    out["tie among the first 64 (first entry's ballot wins)"] = c
    c = steady(kind, 500)
    c[o + 2][1:64:2] = 101
    c[o + 2][64:] = 101
    out["tie among the first 64 (the other way round)"] = c
    c = steady(kind, 3000)                                   # preempted decisions / forwarded proposals: another ballot
    odd = rng.choice(3000, 40, replace=False)
    c[o + 1][odd], c[o + 2][odd] = 1, 101
    c[o + 4][odd] = 2 if kind == DECISIONS else 4
    out["entries of another ballot"] = c
    if kind == PROPOSALS:
        out["every status value"] = steady(kind, 256 * 3, byte=np.arange(256 * 3) % 256)
    for n in range(6):
        out[f"n={n}"] = steady(kind, n)
    for n in (1024, 1025, 1026, 1027):                       # n % 4 = 0 .. 3 across a workgroup's 1024 entries
        out[f"n={n}"] = with_rows(kind, n, 1 + rng.choice(n - 1, 50, replace=False))
    for n in (4000, 4003):                                   # the form boundary: exactly n // 4 rows, and one more
        out[f"n={n}, n // 4 rows"] = with_rows(kind, n, 1 + rng.choice(n - 1, n // 4, replace=False))
        out[f"n={n}, n // 4 + 1 rows"] = with_rows(kind, n, 1 + rng.choice(n - 1, n // 4 + 1, replace=False))
    return out


# ---- engine inputs that bring rows and the columns form about (cases A, B, C) -----------------------------------------
def ahead_of(case, G):
    """How many slots each group is ahead of the others.  Group 0 - the first proposal, and the first decision, of
    every call - is never ahead, so the reference entry is an ordinary group."""
    g = np.arange(G)
    a = np.zeros(G, np.int64)
    if case == "A":
        a[g % 10 == 5] = 1000      # a tenth: rows for those, RECORDS
    elif case == "B":
        a[g % 3 == 1] = 200        # a third: beyond a byte of group 0's slot - COLUMNS; within one of group 7's
        a[7] = 100
    elif case == "C":
        a[g % 2 == 1] = 1000       # half
    elif case is not None:
        raise ValueError(case)
    return a


def ahead_rows(case, G, k, coordinator):
    """Hot-restore rows with acc_slot = next_proposal_slot = 1 + ahead[g]"""
    rows = hri_create(G, k, coordinator)
    a = ahead_of(case, G)
    rows["acc_slot"] = (1 + a).astype(np.int32)
    rows["next_proposal_slot"] = (1 + a).astype(np.int32)
    return rows


def ahead_votes(case, G, members, rnd, coordinator, mix=False):
    """streams.vote_round with every vote's slot and max_cp shifted by its group's lead; case B: group 7's first vote
    swapped to the front, so that the votes' reference lies between the two halves and no vote needs a row."""
    cols = [c.copy() for c in streams.vote_round(G, members, rnd, coordinator, mix=mix)]
    a = ahead_of(case, G)
    cols[3] = (cols[3] + a[cols[0]]).astype(np.int32)
    cols[5] = (cols[5] + a[cols[0]]).astype(np.int32)
    if case == "B":
        j = int(np.argmax(cols[0] == 7))
        for c in cols:
            c[0], c[j] = c[j], c[0]
    return tuple(cols)
