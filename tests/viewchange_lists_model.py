"""The view change in list form (include/gpx_viewchange.h) restated in numpy: dense planes -> lists, for both sides, with
both cuts and from_hit.  The dense call is the specification; this file is what the tests hold the HIP calls against,
computed from the ORACLE's dense calls.

Dense answers are dicts of numpy arrays; planes are flat [W * n], entry j of record i at j * n + i (include/gpx.h)."""
import numpy as np

S_OK, S_WINDOW = 0, 3
V_IGNORED, V_RECORDED, V_ELECTED, V_PREEMPTED = 0, 1, 2, 3
P_NACK, P_TOLOG = 1, 2
TILE = 256                      # GPX_VCL_TILE
HIT_COLS = ("rec", "gidx", "kind", "status", "median", "off", "count")
ENTRY_COLS = ("slot", "kind", "handle", "flags")
PLANES = ("e_slot", "e_kind", "e_handle", "e_flags")


# ---- coordinator side -----------------------------------------------------------------------------------------------------
def dense_from_answer(gidx, answer, W):
    """Engine.prepare_reply's answer ((v_kind, e_median, status), per-record entry lists) as the dense columns."""
    (vk, em, st), lists = answer
    n = len(lists)
    d = dict(n=n, gidx=np.asarray(gidx, np.int32).copy(), v_kind=np.asarray(vk, np.uint8).copy(),
             status=np.asarray(st, np.uint8).copy(), e_median=np.asarray(em, np.int32).copy(),
             e_count=np.array([len(x) for x in lists], np.int32), e_slot=np.zeros(W * n, np.int32),
             e_kind=np.zeros(W * n, np.uint8), e_handle=np.zeros(W * n, np.int64), e_flags=np.zeros(W * n, np.uint8))
    for i, lst in enumerate(lists):
        for j, (s_, k_, h, fl) in enumerate(lst):
            d["e_slot"][j * n + i], d["e_kind"][j * n + i], d["e_handle"][j * n + i], d["e_flags"][j * n + i] = s_, k_, h, fl
    return d


def take(d, idx):
    """The dense answer restricted to the records idx (in that order)."""
    idx = np.asarray(idx, np.int64)
    n, m = d["n"], idx.shape[0]
    W = d["e_slot"].shape[0] // max(n, 1)
    out = {k: d[k][idx].copy() for k in ("gidx", "v_kind", "status", "e_median", "e_count")}
    out["n"] = m
    for nm in PLANES:
        out[nm] = d[nm].reshape(W, n)[:, idx].reshape(-1).copy() if n else d[nm][:0]
    return out


class ReplyModel:
    """gpx_prepare_reply_lists over one dense answer: the hits found once, every cut an index computation."""

    def __init__(self, d, W):
        self.d, self.W, n = d, W, d["n"]
        vk, st = d["v_kind"][:n], d["status"][:n]
        hit = (st != S_OK) | (vk == V_ELECTED) | (vk == V_PREEMPTED)
        self.rec = np.nonzero(hit)[0].astype(np.int32)
        self.cnt = np.clip(d["e_count"][:n][self.rec], 0, W).astype(np.int32)
        self.pre = np.concatenate([[0], np.cumsum(self.cnt)]).astype(np.int64)   # entries before hit q; [-1]: all
        self.n_hits, self.n_entries = int(self.rec.shape[0]), int(self.pre[-1])
        self.classes = dict(n_elected=int((vk == V_ELECTED).sum()), n_preempted=int((vk == V_PREEMPTED).sum()),
                            n_dropped=int((st != S_OK).sum()))
        # the entry rows of all hits, in output order
        q = np.repeat(np.arange(self.n_hits), self.cnt)
        j = np.arange(self.n_entries) - self.pre[q]
        src = j * n + self.rec[q]
        self.entries = {c: d["e_" + c][src] for c in ENTRY_COLS}

    def more(self, from_hit=0, cap_hits=None, cap_entries=None):
        """-> (hits, entries, counts): hit q (from from_hit) fits iff q < cap_hits and h_off + h_count <= cap_entries;
        the first that does not fit ends the output."""
        d = self.d
        cap_hits = self.n_hits if cap_hits is None else cap_hits
        cap_entries = self.n_entries if cap_entries is None else cap_entries
        f = min(from_hit, self.n_hits)
        eb = int(self.pre[f])
        ends = self.pre[f + 1:] - eb                                  # ascending
        k = int(min(cap_hits, np.searchsorted(ends, cap_entries, side="right")))
        k = min(k, self.n_hits - f)
        ed = int(ends[k - 1]) if k else 0
        r = self.rec[f:f + k]
        hits = dict(rec=r.copy(), gidx=d["gidx"][r], kind=d["v_kind"][r], status=d["status"][r], median=d["e_median"][r],
                    off=(self.pre[f:f + k] - eb).astype(np.int32), count=self.cnt[f:f + k].copy())
        entries = {c: a[eb:eb + ed] for c, a in self.entries.items()}
        counts = dict(n_hits=self.n_hits, n_entries=self.n_entries, from_hit=from_hit, hits_done=k, entries_done=ed,
                      **self.classes)
        return hits, entries, counts

    def rounds(self, cap_hits, cap_entries, limit=None):
        """_more from 0 until every hit is out or a round writes nothing -> (hits, entries, hits done, rounds); h_off
        made relative to the concatenated entries."""
        parts, done, ents, nr = [], 0, 0, 0
        while done < self.n_hits and (limit is None or nr < limit):
            h, e, c = self.more(done, cap_hits, cap_entries)
            nr += 1
            if c["hits_done"] == 0:
                break
            h["off"] = h["off"] + np.int32(ents)
            parts.append((h, e))
            done += c["hits_done"]
            ents += c["entries_done"]
        hits = {c: np.concatenate([p[0][c] for p in parts]) if parts else self.more(0, 0, 0)[0][c] for c in HIT_COLS}
        entries = {c: np.concatenate([p[1][c] for p in parts]) if parts else self.more(0, 0, 0)[1][c] for c in ENTRY_COLS}
        return hits, entries, done, nr


def lists_to_planes(hits, entries, n, W):
    """The dense columns the lists stand for: v_kind, status, e_median, e_count and the planes, on the hit records (0
    elsewhere)."""
    out = dict(v_kind=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8), e_median=np.zeros(n, np.int32),
               e_count=np.zeros(n, np.int32), e_slot=np.zeros(W * n, np.int32), e_kind=np.zeros(W * n, np.uint8),
               e_handle=np.zeros(W * n, np.int64), e_flags=np.zeros(W * n, np.uint8))
    r = hits["rec"].astype(np.int64)
    out["v_kind"][r], out["status"][r], out["e_median"][r], out["e_count"][r] = hits["kind"], hits["status"], hits["median"], hits["count"]
    cnt = hits["count"].astype(np.int64)
    assert (cnt >= 0).all() and (cnt <= W).all()
    assert (hits["off"].astype(np.int64) + cnt <= entries["slot"].shape[0]).all() and (hits["off"] >= 0).all()
    q = np.repeat(np.arange(r.shape[0]), cnt)
    j = np.arange(q.shape[0]) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    src = hits["off"].astype(np.int64)[q] + j
    dst = j * n + r[q]
    for c in ENTRY_COLS:
        out["e_" + c][dst] = entries[c][src]
    return out


def dense_on_hits(d, W):
    """What lists_to_planes must give back: the dense answer with everything of a non-hit record, and every plane at or
    beyond a hit's e_count, as 0."""
    n = d["n"]
    vk, st = d["v_kind"][:n], d["status"][:n]
    hit = (st != S_OK) | (vk == V_ELECTED) | (vk == V_PREEMPTED)
    cnt = np.where(hit, np.clip(d["e_count"][:n], 0, W), 0)
    out = dict(v_kind=np.where(hit, vk, 0).astype(np.uint8), status=np.where(hit, st, 0).astype(np.uint8),
               e_median=np.where(hit, d["e_median"][:n], 0).astype(np.int32), e_count=cnt.astype(np.int32))
    live = (np.arange(W)[:, None] < cnt[None, :]).reshape(-1)
    for nm in PLANES:
        out[nm] = np.where(live, d[nm][:W * n], 0).astype(d[nm].dtype)
    return out


def answer_from_lists(n, v_kind, status, hits, entries):
    """Engine.prepare_reply's answer from the lists plus the dense v_kind / status columns."""
    em = np.zeros(n, np.int32)
    lists = [[] for _ in range(n)]
    em[hits["rec"]] = hits["median"]
    for r, o, c in zip(hits["rec"].tolist(), hits["off"].tolist(), hits["count"].tolist()):
        lists[r] = [(int(entries["slot"][x]), int(entries["kind"][x]), int(entries["handle"][x]), int(entries["flags"][x]))
                    for x in range(o, o + c)]
    assert (v_kind[hits["rec"]] == hits["kind"]).all() and (status[hits["rec"]] == hits["status"]).all()
    return (v_kind[:n], em, status[:n]), lists


def same(a, b, what=""):
    for k in a:
        if k == "n":
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x == y).all(), f"{what}: {k} differs" + (
            f" first at {int(np.nonzero(x != y)[0][0])}" if x.shape == y.shape else f" ({x.shape} / {y.shape})")


# ---- acceptor side --------------------------------------------------------------------------------------------------------
def dense_prepare(e, gidx, bnum, bcoord, first_slot):
    """gpx_prepare_batch through the binding's raw call: the five dense columns, p_mask and the three planes."""
    from gigapaxos_amd._abi import _i32, _p
    g = _i32(gidx)
    n = g.shape[0]
    bn, bc, fs = (_i32(np.broadcast_to(np.asarray(x, np.int32), (n,))) for x in (bnum, bcoord, first_slot))
    W, m = int(e.cfg.window), max(n, 1)
    d = dict(n=n, gidx=g, r_bnum=np.zeros(m, np.int32), r_bcoord=np.zeros(m, np.int32), r_gc=np.zeros(m, np.int32),
             r_flags=np.zeros(m, np.uint8), status=np.zeros(m, np.uint8), p_mask=np.zeros(m, np.uint64),
             p_slot=np.zeros(m * W, np.int32), p_bnum=np.zeros(m * W, np.int32), p_bcoord=np.zeros(m * W, np.int32))
    e.lib.check(e.lib.fn["prepare_batch"](e.h, n, _p(g), _p(bn), _p(bc), _p(fs), _p(d["r_bnum"]), _p(d["r_bcoord"]),
                                          _p(d["r_gc"]), _p(d["r_flags"]), _p(d["p_mask"]), _p(d["p_slot"]), _p(d["p_bnum"]),
                                          _p(d["p_bcoord"]), _p(d["status"])), "prepare_batch")
    return d


def prepare_lists(d, W, cap_entries=None):
    """gpx_prepare_lists over a dense answer -> (pv_off[recs_done + 1], slot, bnum, bcoord, counts).  Inside a record
    ascending SIGNED slot (a TreeMap<Integer, ...>)."""
    n = d["n"]
    mask = d["p_mask"][:n]
    bits = ((mask[None, :] >> np.arange(W, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)     # [W][n]
    cnt = bits.sum(axis=0).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    slot = d["p_slot"][:W * n].reshape(W, n)
    # record-major, then signed slot: absent planes last
    key = np.where(bits, slot.astype(np.int64), np.int64(1) << 40)
    order = np.argsort(key, axis=0, kind="stable")                                                     # [W][n]
    w_idx = order.T.reshape(-1)                                                                        # record-major
    i_idx = np.repeat(np.arange(n), W)
    keep = (np.tile(np.arange(W), n) < np.repeat(cnt, W))
    w_idx, i_idx = w_idx[keep], i_idx[keep]
    cols = [d[nm][:W * n].reshape(W, n)[w_idx, i_idx] for nm in ("p_slot", "p_bnum", "p_bcoord")]
    total = int(off[-1])
    cap = total if cap_entries is None else cap_entries
    recs = int(np.searchsorted(off[1:], cap, side="right"))
    ents = int(off[recs])
    st, fl = d["status"][:n], d["r_flags"][:n]
    counts = dict(n_entries=total, recs_done=recs, entries_done=ents, n_dropped=int((st != S_OK).sum()),
                  n_nack=int(((fl & P_NACK) != 0).sum()), n_tolog=int(((fl & P_TOLOG) != 0).sum()))
    return off[:recs + 1].astype(np.int32), cols[0][:ents], cols[1][:ents], cols[2][:ents], counts


def rows_by_signed_slot(rows):
    """Engine.prepare's rows (record, slot, bnum, bcoord) re-sorted by (record, signed slot)."""
    return sorted(rows, key=lambda r: (r[0], r[1]))


def counts_dict(c):
    return {f: int(getattr(c, f)) for f, _ in c._fields_ if f != "reserved"}
