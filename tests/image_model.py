"""The group image format (include/gpx_image.h) restated in numpy, independently of gigapaxos_amd/image.py and of the
kernels: `row_from_dump` builds the canonical row(s) of a group from its canonical dump (gpx_group_dump / orc_group_dump,
docs/HISTORY.md, state dump), `dump_from_rows` is its inverse.  The dump holds everything a row holds except where a ring
entry sits, which slot & (window - 1) determines, and c_pcount, which is the number of outstanding proposals."""
import numpy as np

FORMAT, MAIN, CONT = 1, 1, 2
EXISTS, STOPPED, HASCOORD, PREPARING, CONTINUED = 1, 2, 4, 8, 16
P_PRESENT, P_STOP = 1 << 16, 1 << 17
R_PRESENT, R_STOP, R_HASVALUE = 1, 2, 4
CO_PRESENT = 0x100


def stride(kmax, window):
    """bytes per row: 16 header words, members, node_slots, p_ring, 4-word acc_ring and com_ring entries; whole 64 bytes"""
    return (4 * (16 + 2 * kmax + 9 * window) + 63) // 64 * 64


def cont_words(window):
    return 16 + 8 * window


def _u32(v):
    return int(v) & 0xFFFFFFFF


def parse_dump(dump):
    """the dump's words by name"""
    d = [int(x) for x in dump]
    it = iter(d)
    nx = lambda: next(it)  # noqa: E731
    g = {"exists": nx()}
    if not g["exists"]:
        return g
    g["version"], g["k"] = nx(), nx()
    g["members"] = [nx() for _ in range(g["k"])]
    g["a_slot"], g["a_bnum"], g["a_bcoord"], g["a_gc"], g["stopped"] = nx(), nx(), nx(), nx(), nx()
    g["acc"] = [tuple(nx() for _ in range(4)) for _ in range(nx())]           # slot, bnum, bcoord, stop
    g["com"] = [tuple(nx() for _ in range(6)) for _ in range(nx())]           # slot, bnum, bcoord, median, hasValue, stop
    g["hascoord"] = nx()
    if g["hascoord"]:
        g["c_bnum"], g["c_bcoord"], g["c_next"] = nx(), nx(), nx()
        g["node_slots"] = [nx() for _ in range(g["k"])]
        g["props"] = [tuple(nx() for _ in range(3)) for _ in range(nx())]     # slot, stop, responded mask
        g["active"] = nx()
        if not g["active"]:
            g["armed"], g["heard"] = nx(), nx()
            g["p_handles"] = [(nx(), nx()) for _ in g["props"]]
            g["co"] = [tuple(nx() for _ in range(6)) for _ in range(nx())]    # slot, bnum, bcoord, flags, lo, hi
    assert next(it, None) is None, "words left over"
    return g


def row_from_dump(dump, gidx, my_id, kmax, window):
    """uint8 [1 or 2, stride]: the main row and, for a group that is running for coordinator, its continuation row"""
    g = parse_dump(dump)
    assert g["exists"]
    K, W, k = kmax, window, g["k"]
    sw = stride(K, W) // 4
    prep = bool(g["hascoord"] and not g["active"])
    rows = np.zeros((2 if prep else 1, sw), np.uint32)
    r = rows[0]
    fl = EXISTS | (STOPPED if g["stopped"] else 0) | (HASCOORD if g["hascoord"] else 0) | \
        ((PREPARING | CONTINUED) if prep else 0) | (k << 8)
    r[0:7] = [FORMAT, MAIN, fl, _u32(my_id), K | (W << 16), _u32(gidx), _u32(g["version"])]
    r[7:11] = [_u32(g[f]) for f in ("a_slot", "a_bnum", "a_bcoord", "a_gc")]
    o_mem, o_ns, o_p = 16, 16 + K, 16 + 2 * K
    o_acc, o_com = o_p + W, o_p + 5 * W
    r[o_mem:o_mem + k] = [_u32(m) for m in g["members"]]
    if g["hascoord"]:
        r[11:15] = [_u32(g["c_bnum"]), _u32(g["c_bcoord"]), _u32(g["c_next"]), len(g["props"])]
        r[o_ns:o_ns + k] = [_u32(s) for s in g["node_slots"]]
        for slot, stop, mask in g["props"]:
            r[o_p + (slot & (W - 1))] = P_PRESENT | (P_STOP if stop else 0) | mask
    for slot, bnum, bcoord, stop in g["acc"]:
        x = o_acc + 4 * (slot & (W - 1))
        r[x:x + 4] = [_u32(slot), _u32(bnum), _u32(bcoord), R_PRESENT | (R_STOP if stop else 0)]
    for slot, bnum, bcoord, median, hasv, stop in g["com"]:
        x = slot & (W - 1)
        r[o_com + 4 * x:o_com + 4 * x + 4] = [_u32(slot), _u32(bnum), _u32(bcoord), _u32(median)]
        r[o_acc + 4 * x + 3] |= (R_PRESENT | (R_STOP if stop else 0) | (R_HASVALUE if hasv else 0)) << 8
    if prep:
        c = rows[1]
        c[0], c[1], c[5], c[6] = FORMAT, CONT, _u32(gidx), _u32(g["heard"])
        o_co, o_coh, o_ph = 16, 16 + 4 * W, 16 + 6 * W
        for slot, bnum, bcoord, flags, lo, hi in g["co"]:
            x = slot & (W - 1)
            c[o_co + 4 * x:o_co + 4 * x + 4] = [_u32(slot), _u32(bnum), _u32(bcoord), CO_PRESENT | flags]
            c[o_coh + 2 * x:o_coh + 2 * x + 2] = [_u32(lo), _u32(hi)]
        for (slot, _, _), (lo, hi) in zip(g["props"], g["p_handles"]):
            x = slot & (W - 1)
            c[o_ph + 2 * x:o_ph + 2 * x + 2] = [_u32(lo), _u32(hi)]
    return rows.astype("<u4").view(np.uint8).reshape(rows.shape[0], 4 * sw)


def dump_from_rows(rows, kmax, window):
    """the inverse of row_from_dump: the dump words (int32) of the ONE group in `rows` (uint8 [1 or 2, stride])"""
    K, W = kmax, window
    w = np.ascontiguousarray(rows).view(np.uint8).reshape(-1, stride(K, W)).view("<i4")
    r = [int(x) for x in w[0]]
    assert r[0] == FORMAT and r[1] == MAIN and r[4] == K | (W << 16) and r[15] == 0
    fl = r[2]
    k = (fl >> 8) & 0xFF
    o_mem, o_ns, o_p = 16, 16 + K, 16 + 2 * K
    o_acc, o_com = o_p + W, o_p + 5 * W
    d = [1, r[6], k] + r[o_mem:o_mem + k] + r[7:11] + [int(bool(fl & STOPPED))]
    acc, com = [], []
    for x in range(W):
        s, bn, bc, f = r[o_acc + 4 * x:o_acc + 4 * x + 4]
        if f & R_PRESENT:
            acc.append((s, bn, bc, int(bool(f & R_STOP))))
        if (f >> 8) & R_PRESENT:
            cs, cbn, cbc, med = r[o_com + 4 * x:o_com + 4 * x + 4]
            com.append((cs, cbn, cbc, med, int(bool((f >> 8) & R_HASVALUE)), int(bool((f >> 8) & R_STOP))))
    for lst in (sorted(acc), sorted(com)):
        d += [len(lst)] + [v for t in lst for v in t]
    d.append(int(bool(fl & HASCOORD)))
    if fl & HASCOORD:
        nxt = r[13]
        d += [r[11], r[12], nxt] + r[o_ns:o_ns + k]
        props = []
        for back in range(1, W + 1):
            s = ((nxt - back + 2**31) % 2**32) - 2**31
            e = r[o_p + (s & (W - 1))]
            if e & P_PRESENT:
                props.append((s, int(bool(e & P_STOP)), e & 0xFFFF))
        props.sort()
        assert len(props) == r[14], "c_pcount is the number of outstanding proposals"
        d += [len(props)] + [v for t in props for v in t] + [0 if fl & PREPARING else 1]
        if fl & PREPARING:
            assert fl & CONTINUED and w.shape[0] == 2
            c = [int(x) for x in w[1]]
            assert c[0] == FORMAT and c[1] == CONT and c[5] == r[5]
            o_co, o_coh, o_ph = 16, 16 + 4 * W, 16 + 6 * W
            d += [1, c[6]]
            for s, _, _ in props:
                d += c[o_ph + 2 * (s & (W - 1)):o_ph + 2 * (s & (W - 1)) + 2]
            co = []
            for x in range(W):
                s, bn, bc, f = c[o_co + 4 * x:o_co + 4 * x + 4]
                if f & CO_PRESENT:
                    co.append((s, bn, bc, f & 3, c[o_coh + 2 * x], c[o_coh + 2 * x + 1]))
            co.sort()
            d += [len(co)] + [v for t in co for v in t]
    else:
        assert w.shape[0] == 1
    return np.array(d, np.int64).astype(np.int32)
